// 8f-7 -- ModelNet training pairs on gfx950: SplitSourceRef -> RandomCrop -> RandomTransformSE3_euler -> Resampler ->
// RandomJitter -> ShufflePoints of the reference's ModelNet loader (data_loaders/modelnet.py:102-109,
// data_loaders/modelnet_transforms.py), with counter-based draws.  The draw contract and the float64 apply contract are
// in include/spr.h ("8f-7"); this file follows them operation for operation.
//
// One call, all nb pairs; ONE workgroup of 1024 threads per pair, because every stage of a pair needs an order inside
// the pair's own cloud (two adjacent order statistics of the plane distances, the stable order of the resample keys,
// the stable order of the shuffle keys) and a cloud has at most 8192 points: each order is a bitonic sort of 64-bit
// words in LDS.  Per pair:
//   0   non-finite test, float64 centroid in the contract's fixed order, pose = se3_inv(transform)
//   A   per side: d = dot3(f32(x - c), dir); percentile threshold from the sorted d (ordered-integer image of the
//       doubles); crop flags -> workspace, kept count
//   B   per side: sort (resample key << 32 | raw index) of the kept points; position r < k takes the r-th of them, or
//       an up-sampling extra; LDS atomicMax gives every raw index its LARGEST position
//   C   per side: sort (shuffle key << 32 | position); output j gathers position perm[j]: transform (source), jitter,
//       overlap flag, raw index; the inverse permutation -> workspace
//   D   correspondences: raw indices selected on both sides, ascending, compacted with a workgroup scan
// The operator moves a few MB per step: its floor is the ~400 barriers of the six sorts of a pair, not bandwidth.
#include <cmath>

#include "philox.h"
#include "spr_common.h"

namespace spr {
namespace {

constexpr int kMnThreads = 1024;
constexpr int kMnMaxLen = 8192;   // points per cloud, and the largest k
constexpr unsigned long long kMnLast = ~0ull;

__device__ __forceinline__ double mn_dot3(double a0, double b0, double a1, double b1, double a2, double b2) {
  return __dadd_rn(__dadd_rn(__dmul_rn(a0, b0), __dmul_rn(a1, b1)), __dmul_rn(a2, b2));
}
__device__ __forceinline__ bool mn_finite(float v) { return fabsf(v) <= 3.4028235e38f; }

// doubles <-> unsigned integers in the same order
__device__ __forceinline__ unsigned long long mn_ordered(double d) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(d);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double mn_unordered(unsigned long long o) {
  return __longlong_as_double((long long)((o >> 63) ? (o ^ 0x8000000000000000ull) : ~o));
}

// ascending bitonic sort of a[0 .. p2), p2 a power of two >= 2, by the whole workgroup; ends with a barrier
__device__ void mn_sort(unsigned long long* a, int p2) {
  __syncthreads();
  for (int k2 = 2; k2 <= p2; k2 <<= 1) {
    for (int j = k2 >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < (p2 >> 1); t += blockDim.x) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
        const unsigned long long x = a[i], y = a[l];
        if ((x > y) == ((i & k2) == 0)) a[i] = y, a[l] = x;
      }
      __syncthreads();
    }
  }
}

__device__ __forceinline__ int mn_pow2(int n) {
  int p = 2;
  while (p < n) p <<= 1;
  return p;
}

// One step of a stable workgroup compaction: the output slot of this thread's flagged element; *base advances by the
// step's count.  swave: one int per wave.  Contains three barriers; every thread of the workgroup calls it.
__device__ __forceinline__ int mn_slot(bool f, int* swave, int* base) {
  const unsigned long long bal = __ballot(f);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) swave[wv] = __popcll(bal);
  __syncthreads();
  int off = *base, tot = 0;
  for (int w = 0; w < (int)(blockDim.x >> 6); ++w) {
    if (w < wv) off += swave[w];
    tot += swave[w];
  }
  __syncthreads();
  if (threadIdx.x == 0) *base += tot;
  __syncthreads();
  return off + __popcll(bal & ((1ull << lane) - 1ull));
}

struct MnDraws {
  const unsigned int* rkeys;   // [2, n_total]
  const unsigned int* extra;   // [2, nb k]
  const float* noise;          // [2, nb k, 3]
  const unsigned int* skeys;   // [2, nb k]
};

// crop mode of a side from its p_keep: 0 keep all, 1 the half space d > 0, 2 the percentile
__host__ __device__ inline int mn_mode(float p) { return p == 1.0f ? 0 : (p == 0.5f ? 1 : 2); }

// Dynamic LDS: sort words [p2] u64, then the position maps [2][map_len] i32.
__global__ __launch_bounds__(kMnThreads) void k_modelnet_pairs(
    const float* __restrict__ xyz, const int* __restrict__ cu, int n_total, int nb, int max_len, int p2_max, float p_src,
    float p_tgt, double q_src, double q_tgt, int k, float scale, float clip, const float* __restrict__ transform,
    const double* __restrict__ dirs, uint64_t seed, const uint64_t* __restrict__ pair_key, MnDraws dr,
    float* __restrict__ src_xyz, float* __restrict__ tgt_xyz, float* __restrict__ pose,
    unsigned char* __restrict__ src_overlap, unsigned char* __restrict__ tgt_overlap, int* __restrict__ src_index,
    int* __restrict__ tgt_index, int* __restrict__ corr, int* __restrict__ corr_count, int* __restrict__ status,
    unsigned char* __restrict__ kept, int* __restrict__ rs, int* __restrict__ invp) {
  extern __shared__ unsigned long long mn_lds[];
  unsigned long long* a = mn_lds;
  int* map = (int*)(mn_lds + p2_max);   // [2][max_len]
  __shared__ double ssum[3][16];
  __shared__ double sthr;
  __shared__ int sbad, skept[2], swave[16], sbase;

  const int b = blockIdx.x, tid = threadIdx.x;
  const int beg = cu[b];
  int n = cu[b + 1] - beg;
  const size_t nk = (size_t)nb * (size_t)k, ob = (size_t)b * (size_t)k;
  // a cloud outside the call's promise (or outside the packed array) is not touched: status 3
  const bool legal = n >= 0 && n <= max_len && beg >= 0 && (long)beg + n <= (long)n_total;
  if (!legal) n = 0;
  const float* x = xyz + 3 * (size_t)(legal ? beg : 0);
  const uint64_t pk = pair_key ? pair_key[b] : 0;

  if (tid == 0) sbad = 0, skept[0] = 0, skept[1] = 0;
  __syncthreads();

  // ---- 0: non-finite test, centroid, pose ----------------------------------------------------------------------------
  double sum[3] = {0.0, 0.0, 0.0};
  bool bad = false;
  for (int i = tid; i < n; i += kMnThreads) {
    const float px = x[3 * (size_t)i], py = x[3 * (size_t)i + 1], pz = x[3 * (size_t)i + 2];
    bad = bad || !(mn_finite(px) && mn_finite(py) && mn_finite(pz));
    sum[0] = __dadd_rn(sum[0], (double)px), sum[1] = __dadd_rn(sum[1], (double)py), sum[2] = __dadd_rn(sum[2], (double)pz);
  }
  if (tid < 12) bad = bad || !mn_finite(transform[12 * (size_t)b + tid]);
  if (tid < 6) bad = bad || !(fabs(dirs[6 * (size_t)b + tid]) <= 1.7976931348623157e308);
  if (bad) atomicOr(&sbad, 1);
  for (int d = 0; d < 3; ++d) {
    const double w = wave_sum_d(sum[d]);
    if ((tid & 63) == 0) ssum[d][tid >> 6] = w;
  }
  __syncthreads();
  double c[3];
  for (int d = 0; d < 3; ++d) {
    double s = 0.0;
    for (int w = 0; w < kMnThreads / 64; ++w) s = __dadd_rn(s, ssum[d][w]);
    c[d] = n > 0 ? (double)(float)__ddiv_rn(s, (double)n) : 0.0;
  }
  double T[12];
  for (int e = 0; e < 12; ++e) T[e] = (double)transform[12 * (size_t)b + e];
  if (tid < 3) {   // pose = f32([R^T | -(R^T t)])
    float* o = pose + 12 * (size_t)b + 4 * tid;
    o[0] = (float)T[tid], o[1] = (float)T[4 + tid], o[2] = (float)T[8 + tid];
    o[3] = (float)-mn_dot3(T[tid], T[3], T[4 + tid], T[7], T[8 + tid], T[11]);
  }
  const bool nonfinite = sbad != 0;

  // ---- A: crop flags of both sides -------------------------------------------------------------------------------------
  for (int side = 0; side < 2 && !nonfinite; ++side) {
    const int mode = mn_mode(side ? p_tgt : p_src);
    const double* dir = dirs + 6 * (size_t)b + 3 * side;
    const double d0 = dir[0], d1 = dir[1], d2 = dir[2];
    auto dist = [&](int i) {
      const double v0 = (double)(float)__dsub_rn((double)x[3 * (size_t)i], c[0]);
      const double v1 = (double)(float)__dsub_rn((double)x[3 * (size_t)i + 1], c[1]);
      const double v2 = (double)(float)__dsub_rn((double)x[3 * (size_t)i + 2], c[2]);
      return mn_dot3(v0, d0, v1, d1, v2, d2);
    };
    double thr = 0.0;
    if (mode == 2 && n > 0) {
      const int p2 = mn_pow2(n);
      for (int i = tid; i < p2; i += kMnThreads) a[i] = i < n ? mn_ordered(dist(i)) : kMnLast;
      mn_sort(a, p2);
      if (tid == 0) {   // numpy's 'linear' percentile
        const double h = __dmul_rn((double)(n - 1), __ddiv_rn(side ? q_tgt : q_src, 100.0));
        int lo = (int)floor(h);
        lo = lo < 0 ? 0 : (lo > n - 1 ? n - 1 : lo);
        const int hi = lo + 1 > n - 1 ? n - 1 : lo + 1;
        const double t = __dsub_rn(h, (double)lo), va = mn_unordered(a[lo]), vb = mn_unordered(a[hi]);
        const double diff = __dsub_rn(vb, va);
        sthr = t < 0.5 ? __dadd_rn(va, __dmul_rn(diff, t)) : __dsub_rn(vb, __dmul_rn(diff, __dsub_rn(1.0, t)));
      }
      __syncthreads();
      thr = sthr;
    }
    int cnt = 0;
    for (int i = tid; i < n; i += kMnThreads) {
      const bool keep = mode == 0 || dist(i) > thr;
      kept[(size_t)side * n_total + beg + i] = keep ? 1 : 0;
      cnt += keep ? 1 : 0;
    }
    if (cnt) atomicAdd(&skept[side], cnt);
    __syncthreads();   // the flags and the count are complete; `a` and sthr are free again
  }
  const int st = !legal ? 3 : (nonfinite ? 1 : ((skept[0] == 0 || skept[1] == 0) ? 2 : 0));
  if (tid == 0) status[b] = st;
  if (st != 0) {   // no points: zeros, no correspondences
    for (int j = tid; j < k; j += kMnThreads) {
      for (int e = 0; e < 3; ++e) src_xyz[3 * (ob + j) + e] = 0.f, tgt_xyz[3 * (ob + j) + e] = 0.f;
      src_overlap[ob + j] = 0, tgt_overlap[ob + j] = 0;
      src_index[ob + j] = 0, tgt_index[ob + j] = 0;
    }
    if (tid == 0) corr_count[b] = 0;
    return;
  }

  // ---- B, C per side -----------------------------------------------------------------------------------------------------
  for (int i = tid; i < 2 * max_len; i += kMnThreads) map[i] = -1;
  for (int side = 0; side < 2; ++side) {
    const int nkept = skept[side];
    const unsigned char* mine = kept + (size_t)side * n_total + beg;
    const unsigned char* other = kept + (size_t)(1 - side) * n_total + beg;
    int* smap = map + side * max_len;
    int* srs = rs + side * nk + ob;
    int* sinv = invp + side * nk + ob;
    // B: the kept points in the stable ascending order of their resample keys
    const int p2 = mn_pow2(n);
    for (int i = tid; i < p2; i += kMnThreads) {
      unsigned long long w = kMnLast;
      if (i < n && mine[i]) {
        const uint32_t key = dr.rkeys ? dr.rkeys[(size_t)side * n_total + beg + i]
                                      : philox_block(seed, pk, side, (uint32_t)i, kTagMnResample).w[0];
        w = ((unsigned long long)key << 32) | (unsigned int)i;
      }
      a[i] = w;
    }
    mn_sort(a, p2);
    if (nkept < k) {   // up-sampling: the extras count the kept points in ascending raw order -> sinv (free until C)
      if (tid == 0) sbase = 0;
      __syncthreads();
      for (int i0 = 0; i0 < n; i0 += kMnThreads) {
        const int i = i0 + tid;
        const bool f = i < n && mine[i];
        const int o = mn_slot(f, swave, &sbase);
        if (f && o < k) sinv[o] = i;   // o < nkept < k
      }
      __syncthreads();
    }
    for (int r = tid; r < k; r += kMnThreads) {
      int raw;
      if (r < nkept) {
        raw = (int)(unsigned int)(a[r] & 0xffffffffull);
      } else {
        const uint32_t w = dr.extra ? dr.extra[side * nk + ob + (r - nkept)]
                                    : philox_block(seed, pk, side, (uint32_t)(r - nkept), kTagMnExtra).w[0];
        const double u = __dmul_rn((double)(w >> 9) + 0.5, 1.1920928955078125e-7);
        int pick = (int)floor(__dmul_rn(u, (double)nkept));
        pick = pick < 0 ? 0 : (pick > nkept - 1 ? nkept - 1 : pick);
        raw = sinv[pick];
      }
      raw = (raw >= 0 && raw < n) ? raw : 0;   // not reachable: both lists hold kept points
      srs[r] = raw;
      atomicMax(&smap[raw], r);
    }
    __syncthreads();
    // C: the k positions in the stable ascending order of their shuffle keys
    const int pk2 = mn_pow2(k);
    for (int j = tid; j < pk2; j += kMnThreads) {
      unsigned long long w = kMnLast;
      if (j < k) {
        const uint32_t key = dr.skeys ? dr.skeys[side * nk + ob + j]
                                      : philox_block(seed, pk, side, (uint32_t)j, kTagMnShuffle).w[0];
        w = ((unsigned long long)key << 32) | (unsigned int)j;
      }
      a[j] = w;
    }
    mn_sort(a, pk2);
    float* oxyz = side ? tgt_xyz : src_xyz;
    unsigned char* oov = side ? tgt_overlap : src_overlap;
    int* oidx = side ? tgt_index : src_index;
    for (int j = tid; j < k; j += kMnThreads) {
      int r = (int)(unsigned int)(a[j] & 0xffffffffull);
      r = r < k ? r : 0;   // not reachable
      sinv[r] = j;
      const int raw = srs[r];
      float p[3] = {x[3 * (size_t)raw], x[3 * (size_t)raw + 1], x[3 * (size_t)raw + 2]};
      if (side == 0) {
        const double xd = (double)p[0], yd = (double)p[1], zd = (double)p[2];
        for (int e = 0; e < 3; ++e)
          p[e] = (float)__dadd_rn(mn_dot3(T[4 * e], xd, T[4 * e + 1], yd, T[4 * e + 2], zd), T[4 * e + 3]);
      }
      float nz[3];
      if (dr.noise) {
        const float* g = dr.noise + 3 * (side * nk + ob + r);
        nz[0] = g[0], nz[1] = g[1], nz[2] = g[2];
      } else {
        philox_normal3(philox_block(seed, pk, side, (uint32_t)r, kTagMnNoise), nz);
      }
      for (int e = 0; e < 3; ++e) {
        const float v = fminf(fmaxf(__fmul_rn(nz[e], scale), -clip), clip);
        oxyz[3 * (ob + j) + e] = __fadd_rn(p[e], v);
      }
      oov[ob + j] = other[raw];
      oidx[ob + j] = raw;
    }
    __syncthreads();   // `a` is free again; sinv is complete
  }

  // ---- D: correspondences, ascending raw index ------------------------------------------------------------------------
  if (tid == 0) sbase = 0;
  __syncthreads();
  const int* inv0 = invp + ob;
  const int* inv1 = invp + nk + ob;
  for (int i0 = 0; i0 < n; i0 += kMnThreads) {
    const int i = i0 + tid;
    const int ra = i < n ? map[i] : -1, rb = i < n ? map[max_len + i] : -1;
    const bool f = ra >= 0 && rb >= 0;
    const int o = mn_slot(f, swave, &sbase);
    if (f && o < k) {   // always: every survivor owns a source position of its own
      corr[ob + o] = inv0[ra];
      corr[nk + ob + o] = inv1[rb];
    }
  }
  if (tid == 0) corr_count[b] = sbase < k ? sbase : k;
}

// the per-point draws as buffers: what k_modelnet_pairs generates inline
__global__ __launch_bounds__(256) void k_modelnet_draw(int n_total, int nb, int k, const int* __restrict__ cu,
                                                       uint64_t seed, const uint64_t* __restrict__ pair_key,
                                                       unsigned int* __restrict__ rkeys, unsigned int* __restrict__ extra,
                                                       float* __restrict__ noise, unsigned int* __restrict__ skeys) {
  const size_t nk = (size_t)nb * (size_t)k;
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int side = blockIdx.y;
  if (rkeys && g < (size_t)n_total) {
    const int b = find_segment(cu, nb, (int)g);
    rkeys[(size_t)side * n_total + g] = philox_block(seed, pair_key[b], side, (uint32_t)((int)g - cu[b]), kTagMnResample).w[0];
  }
  if (g < nk) {
    const int b = (int)(g / (size_t)k);
    const uint32_t e = (uint32_t)(g - (size_t)b * (size_t)k);
    const uint64_t pk = pair_key[b];
    if (extra) extra[side * nk + g] = philox_block(seed, pk, side, e, kTagMnExtra).w[0];
    if (skeys) skeys[side * nk + g] = philox_block(seed, pk, side, e, kTagMnShuffle).w[0];
    if (noise) {
      float nz[3];
      philox_normal3(philox_block(seed, pk, side, e, kTagMnNoise), nz);
      float* o = noise + 3 * (side * nk + g);
      o[0] = nz[0], o[1] = nz[1], o[2] = nz[2];
    }
  }
}

struct MnWs {
  unsigned char* kept;   // [2, n_total] crop flags
  int *rs, *invp;        // [2, nb k] raw index of every resampled position; output slot of every position
};
MnWs mn_layout(Workspace& w, int n_total, int nb, int k) {
  const size_t N = n_total > 0 ? (size_t)n_total : 1, K = (size_t)(nb > 0 ? nb : 1) * (size_t)(k > 0 ? k : 1);
  MnWs l;
  l.kept = w.take<unsigned char>(2 * N);
  l.rs = w.take<int>(2 * K);
  l.invp = w.take<int>(2 * K);
  return l;
}

// ---- pair decisions: float64 on the host -----------------------------------------------------------------------------
double mn_u64(uint32_t w) { return ((double)(w >> 9) + 0.5) * 1.1920928955078125e-7; }
constexpr double kMnPi = 3.14159265358979323846;

void mn_decide(uint64_t seed, uint64_t pair_key, double rot_mag, double trans_mag, double* dirs, float* tf) {
  if (dirs) {
    for (int side = 0; side < 2; ++side) {   // uniform_2_sphere
      const Philox4 b = philox_block(seed, pair_key, side, 0, kTagMnPair);
      const double phi = 2.0 * kMnPi * mn_u64(b.w[0]), z = 2.0 * mn_u64(b.w[1]) - 1.0, th = std::acos(z);
      dirs[3 * side + 0] = std::sin(th) * std::cos(phi);
      dirs[3 * side + 1] = std::sin(th) * std::sin(phi);
      dirs[3 * side + 2] = std::cos(th);
    }
  }
  if (!tf) return;
  const Philox4 b1 = philox_block(seed, pair_key, 0, 1, kTagMnPair), b2 = philox_block(seed, pair_key, 0, 2, kTagMnPair);
  const double ax = mn_u64(b1.w[0]) * kMnPi * rot_mag / 180.0, ay = mn_u64(b1.w[1]) * kMnPi * rot_mag / 180.0,
               az = mn_u64(b1.w[2]) * kMnPi * rot_mag / 180.0;
  const double cx = std::cos(ax), sx = std::sin(ax), cy = std::cos(ay), sy = std::sin(ay), cz = std::cos(az),
               sz = std::sin(az);
  const double Rx[9] = {1, 0, 0, 0, cx, -sx, 0, sx, cx}, Ry[9] = {cy, 0, sy, 0, 1, 0, -sy, 0, cy},
               Rz[9] = {cz, -sz, 0, sz, cz, 0, 0, 0, 1};
  double A[9], R[9];   // R = (Rx Ry) Rz, every entry ((a0 b0 + a1 b1) + a2 b2)
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) A[3 * i + j] = (Rx[3 * i] * Ry[j] + Rx[3 * i + 1] * Ry[3 + j]) + Rx[3 * i + 2] * Ry[6 + j];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) R[3 * i + j] = (A[3 * i] * Rz[j] + A[3 * i + 1] * Rz[3 + j]) + A[3 * i + 2] * Rz[6 + j];
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) tf[4 * i + j] = (float)R[3 * i + j];
    tf[4 * i + 3] = (float)(-trans_mag + 2.0 * trans_mag * mn_u64(b2.w[i]));
  }
}

}  // namespace
}  // namespace spr

using namespace spr;

extern "C" int spr_modelnet_draw(uint64_t seed, const uint64_t* pair_key_host, int nb, double rot_mag, double trans_mag,
                                 double* dirs_host, float* transform_host, const uint64_t* pair_key, const int* cu,
                                 int n_total, int k, unsigned int* rkeys, unsigned int* extra, float* noise,
                                 unsigned int* skeys, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPR_REQUIRE(nb >= 0 && n_total >= 0, "modelnet_draw: negative size (nb=%d n_total=%d)", nb, n_total);
  SPR_REQUIRE(std::isfinite(rot_mag) && std::isfinite(trans_mag), "modelnet_draw: rot_mag and trans_mag must be finite");
  if (dirs_host || transform_host) {
    SPR_REQUIRE(nb == 0 || pair_key_host, "modelnet_draw: pair_key_host must not be null");
    for (int b = 0; b < nb; ++b) {
      SPR_REQUIRE(pair_key_host[b] < (1ull << 63), "modelnet_draw: pair_key[%d] must be below 2^63", b);
      mn_decide(seed, pair_key_host[b], rot_mag, trans_mag, dirs_host ? dirs_host + 6 * (size_t)b : nullptr,
                transform_host ? transform_host + 12 * (size_t)b : nullptr);
    }
  }
  if (!rkeys && !extra && !noise && !skeys) return 0;
  SPR_REQUIRE(k >= 1 && k <= kMnMaxLen, "modelnet_draw: k must be in [1, %d], got %d", kMnMaxLen, k);
  SPR_REQUIRE(n_total <= (1 << 26) && (size_t)nb * (size_t)k <= ((size_t)1 << 26),
              "modelnet_draw: at most 2^26 input points and 2^26 output points per call");
  SPR_REQUIRE(nb > 0 || n_total == 0, "modelnet_draw: points without pairs (nb=0 n_total=%d)", n_total);
  if (nb == 0) return 0;
  SPR_REQUIRE(pair_key && cu, "modelnet_draw: pair_key and cu (device) must not be null");
  const size_t most = (size_t)nb * (size_t)k > (size_t)n_total ? (size_t)nb * (size_t)k : (size_t)n_total;
  hipLaunchKernelGGL(k_modelnet_draw, dim3(cdiv((long)most, 256), 2), dim3(256), 0, stream, n_total, nb, k, cu, seed,
                     pair_key, rkeys, extra, noise, skeys);
  SPR_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t spr_modelnet_pairs_workspace_size(int n_total, int nb, int k) {
  if (n_total < 0 || nb < 0 || k < 0) return 0;
  return measure(mn_layout, n_total, nb, k);
}

extern "C" int spr_modelnet_pairs(const float* xyz, const int* cu, int n_total, int nb, int max_len_host, float p_src,
                                  float p_tgt, double q_src, double q_tgt, int k, float scale, float clip,
                                  const float* transform, const double* dirs, uint64_t seed, const uint64_t* pair_key,
                                  const unsigned int* rkeys, const unsigned int* extra, const float* noise,
                                  const unsigned int* skeys, float* src_xyz, float* tgt_xyz, float* pose,
                                  unsigned char* src_overlap, unsigned char* tgt_overlap, int* src_index,
                                  int* tgt_index, int* corr, int* corr_count, int* status, void* ws, size_t ws_bytes,
                                  void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPR_REQUIRE(nb >= 0 && n_total >= 0 && max_len_host >= 0, "modelnet_pairs: negative size (nb=%d n_total=%d max_len=%d)",
              nb, n_total, max_len_host);
  SPR_REQUIRE(max_len_host <= kMnMaxLen, "modelnet_pairs: a cloud of %d points; at most %d are supported", max_len_host,
              kMnMaxLen);
  SPR_REQUIRE(k >= 1 && k <= kMnMaxLen, "modelnet_pairs: k must be in [1, %d], got %d", kMnMaxLen, k);
  SPR_REQUIRE(p_src > 0.f && p_src <= 1.f && p_tgt > 0.f && p_tgt <= 1.f,
              "modelnet_pairs: p_keep must be in (0, 1], got %g / %g", (double)p_src, (double)p_tgt);
  SPR_REQUIRE((mn_mode(p_src) != 2 || (q_src >= 0.0 && q_src <= 100.0)) && (mn_mode(p_tgt) != 2 || (q_tgt >= 0.0 && q_tgt <= 100.0)),
              "modelnet_pairs: the percentile must be in [0, 100], got %g / %g", q_src, q_tgt);
  SPR_REQUIRE(scale >= 0.f && scale < 3.0e38f && clip >= 0.f && clip < 3.0e38f,
              "modelnet_pairs: scale and clip must be finite and >= 0");
  SPR_REQUIRE(n_total <= (1 << 26) && (size_t)nb * (size_t)k <= ((size_t)1 << 26),
              "modelnet_pairs: at most 2^26 input points and 2^26 output points per call");
  SPR_REQUIRE(nb > 0 || n_total == 0, "modelnet_pairs: points without pairs (nb=0 n_total=%d)", n_total);
  if (nb == 0) return 0;
  SPR_REQUIRE(cu && transform && dirs, "modelnet_pairs: cu, transform and dirs must not be null");
  SPR_REQUIRE(n_total == 0 || xyz, "modelnet_pairs: null xyz with n_total=%d", n_total);
  SPR_REQUIRE(src_xyz && tgt_xyz && pose && src_overlap && tgt_overlap && src_index && tgt_index && corr && corr_count && status,
              "modelnet_pairs: null output pointer");
  SPR_REQUIRE((rkeys && extra && noise && skeys) || pair_key,
              "modelnet_pairs: pair_key must not be null when draws are generated inline");
  Workspace w(ws, ws_bytes);
  const auto [kept, rs, invp] = mn_layout(w, n_total, nb, k);
  SPR_REQUIRE(ws != nullptr && w.ok(), "modelnet_pairs: workspace too small");

  int p2 = 2;
  while (p2 < max_len_host || p2 < k) p2 <<= 1;
  const int map_len = max_len_host > 0 ? max_len_host : 1;
  const size_t lds = 8 * (size_t)p2 + 8 * (size_t)map_len;
  if (int rc = ensure_dyn_lds((const void*)k_modelnet_pairs, (int)lds)) return rc;
  const MnDraws dr = {rkeys, extra, noise, skeys};
  hipLaunchKernelGGL(k_modelnet_pairs, dim3(nb), dim3(kMnThreads), lds, stream, xyz, cu, n_total, nb, map_len, p2, p_src,
                     p_tgt, q_src, q_tgt, k, scale, clip, transform, dirs, seed, pair_key, dr, src_xyz, tgt_xyz, pose,
                     src_overlap, tgt_overlap, src_index, tgt_index, corr, corr_count, status, kept, rs, invp);
  SPR_LAUNCH_CHECK();
  return 0;
}
