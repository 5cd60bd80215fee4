// 8f-6 -- training augmentation of all pairs of a step on gfx950: RigidPerturb -> Jitter -> ShufflePoints ->
// RandomSwap of the reference's 3DMatch / KITTI loaders (data_loaders/transforms.py:15-179), with counter-based
// draws.  The draw contract and the float64 apply contract are in include/spr.h ("8f-6"); this file follows them
// operation for operation.
//
// One call, all B pairs, clouds stacked [src_0 .. src_{B-1}, tgt_0 .. tgt_{B-1}] (cloud c, global point g):
//   k_aug_keys    sort key (c << 32 | shuffle key) and value g per point; the key is word 0 of the point's tag-2
//                 Philox block unless the caller hands keys in
//   rocPRIM radix sort (stable) over 32 + log2(2 B) bits: the sorted run of cloud c IS its permutation
//   k_aug_layout  output cu arrays: min(len, max_pts) per cloud, sides exchanged where the pair swaps
//   k_aug_pose    one workgroup per pair: non-finite test of both clouds, float64 centroid of the perturbed one,
//                 P' = C^-1 P C, pose' and the swap's inverse -- the whole pose algebra, in one thread at the end
//   k_aug_gather  ONE pass over the sorted order: rank -> keep or cut, inverse permutation, load the 12-byte point,
//                 transform it if its cloud is the perturbed one, add the (inline Philox) noise, store point, mask
//                 and permutation entry in the (possibly swapped) output slot
//   k_aug_cmark -> rocPRIM exclusive scan -> k_aug_ccompact: correspondences through the inverse permutation,
//                 stable compaction inside each pair's own column run (as gt_overlap.hip does).
// The operator moves a few MB per step: its floor is launch latency plus the sort, not bandwidth.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <cmath>

#include "philox.h"
#include "spr_common.h"

namespace spr {
namespace {

// Philox4x32-10, the block layout, the stream tags and the float32 normal triple: philox.h
__device__ __forceinline__ void aug_noise(uint64_t seed, uint64_t pair_key, int side, int i, float* n) {
  philox_normal3(philox_block(seed, pair_key, side, (uint32_t)i, kTagNoise), n);
}

__device__ __forceinline__ uint32_t aug_key(uint64_t seed, uint64_t pair_key, int side, int i) {
  return philox_block(seed, pair_key, side, (uint32_t)i, kTagKey).w[0];
}

// cloud c of the stacked sequence: (pair, side, first global point, length)
struct AugCloud {
  int pair, side, beg, len;
};
__device__ __forceinline__ AugCloud aug_cloud(int c, int nb, int ns, const int* __restrict__ src_cu,
                                              const int* __restrict__ tgt_cu) {
  AugCloud a;
  a.side = c >= nb ? 1 : 0;
  a.pair = a.side ? c - nb : c;
  const int* cu = a.side ? tgt_cu : src_cu;
  a.beg = (a.side ? ns : 0) + cu[a.pair];
  a.len = cu[a.pair + 1] - cu[a.pair];
  return a;
}
// cloud of global point g
__device__ __forceinline__ int aug_cloud_of(int g, int nb, int ns, const int* __restrict__ src_cu,
                                            const int* __restrict__ tgt_cu) {
  return g < ns ? find_segment(src_cu, nb, g) : nb + find_segment(tgt_cu, nb, g - ns);
}

__global__ __launch_bounds__(256) void k_aug_keys(int np, int ns, int nb, const int* __restrict__ src_cu,
                                                  const int* __restrict__ tgt_cu, uint64_t seed,
                                                  const uint64_t* __restrict__ pair_key,
                                                  const unsigned int* __restrict__ keys,
                                                  unsigned long long* __restrict__ skey,
                                                  unsigned int* __restrict__ sval) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= np) return;
  const int c = aug_cloud_of(g, nb, ns, src_cu, tgt_cu);
  const AugCloud a = aug_cloud(c, nb, ns, src_cu, tgt_cu);
  const uint32_t k = keys ? keys[g] : aug_key(seed, pair_key[a.pair], a.side, g - a.beg);
  skey[g] = ((unsigned long long)c << 32) | k;
  sval[g] = (unsigned int)g;
}

// the draws as buffers: what k_aug_keys / k_aug_gather generate inline
__global__ __launch_bounds__(256) void k_aug_draw(int np, int ns, int nb, const int* __restrict__ src_cu,
                                                  const int* __restrict__ tgt_cu, uint64_t seed,
                                                  const uint64_t* __restrict__ pair_key, float* __restrict__ noise,
                                                  unsigned int* __restrict__ keys) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= np) return;
  const int c = aug_cloud_of(g, nb, ns, src_cu, tgt_cu);
  const AugCloud a = aug_cloud(c, nb, ns, src_cu, tgt_cu);
  const uint64_t pk = pair_key[a.pair];
  if (keys) keys[g] = aug_key(seed, pk, a.side, g - a.beg);
  if (noise) {
    float n[3];
    aug_noise(seed, pk, a.side, g - a.beg, n);
    noise[3 * (size_t)g + 0] = n[0];
    noise[3 * (size_t)g + 1] = n[1];
    noise[3 * (size_t)g + 2] = n[2];
  }
}

__global__ void k_aug_layout(int nb, int max_pts, const int* __restrict__ src_cu, const int* __restrict__ tgt_cu,
                             const unsigned char* __restrict__ flags, int* __restrict__ out_src_cu,
                             int* __restrict__ out_tgt_cu) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  int os = 0, ot = 0;
  out_src_cu[0] = 0;
  out_tgt_cu[0] = 0;
  for (int b = 0; b < nb; ++b) {
    const int ls = min(src_cu[b + 1] - src_cu[b], max_pts), lt = min(tgt_cu[b + 1] - tgt_cu[b], max_pts);
    const bool swap = (flags[b] & 2) != 0;
    os += swap ? lt : ls;
    ot += swap ? ls : lt;
    out_src_cu[b + 1] = os;
    out_tgt_cu[b + 1] = ot;
  }
}

__device__ __forceinline__ double aug_dot3(double a0, double b0, double a1, double b1, double a2, double b2) {
  return __dadd_rn(__dadd_rn(__dmul_rn(a0, b0), __dmul_rn(a1, b1)), __dmul_rn(a2, b2));
}
// [3,4] row-major; out = f32-rounded values held in double
__device__ void aug_cat(const double* A, const double* B, double* o) {
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) o[4 * i + j] = aug_dot3(A[4 * i], B[j], A[4 * i + 1], B[4 + j], A[4 * i + 2], B[8 + j]);
    o[4 * i + 3] = __dadd_rn(aug_dot3(A[4 * i], B[3], A[4 * i + 1], B[7], A[4 * i + 2], B[11]), A[4 * i + 3]);
  }
}
__device__ void aug_inv(const double* A, double* o) {
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) o[4 * i + j] = A[4 * j + i];
    o[4 * i + 3] = -aug_dot3(A[i], A[3], A[4 + i], A[7], A[8 + i], A[11]);
  }
}
__device__ __forceinline__ void aug_round(double* A) {
  for (int k = 0; k < 12; ++k) A[k] = (double)(float)A[k];
}
__device__ __forceinline__ bool aug_finite(float v) { return fabsf(v) <= 3.4028235e38f; }

// One workgroup per pair.  T [nb,12]: P' of the pair (what its perturbed cloud is transformed by).
__global__ __launch_bounds__(1024) void k_aug_pose(int nb, int ns, const float* __restrict__ src_xyz,
                                                   const int* __restrict__ src_cu, const float* __restrict__ tgt_xyz,
                                                   const int* __restrict__ tgt_cu, const float* __restrict__ pose,
                                                   const float* __restrict__ perturb,
                                                   const unsigned char* __restrict__ flags, int mode,
                                                   float* __restrict__ T, float* __restrict__ out_pose,
                                                   int* __restrict__ status) {
  const int b = blockIdx.x;
  const int f = flags[b];
  const int pside = (f & 1) ? 0 : 1;
  __shared__ double ssum[3][16];
  __shared__ int sbad;
  if (threadIdx.x == 0) sbad = 0;
  __syncthreads();
  double sum[3] = {0.0, 0.0, 0.0};
  bool bad = false;
  for (int side = 0; side < 2; ++side) {
    const int* cu = side ? tgt_cu : src_cu;
    const float* xyz = side ? tgt_xyz : src_xyz;
    const bool acc = mode == SPR_AUG_SMALL && side == pside;
    for (int p = cu[b] + threadIdx.x; p < cu[b + 1]; p += blockDim.x) {
      const float x = xyz[3 * (size_t)p], y = xyz[3 * (size_t)p + 1], z = xyz[3 * (size_t)p + 2];
      bad = bad || !(aug_finite(x) && aug_finite(y) && aug_finite(z));
      if (acc) sum[0] += (double)x, sum[1] += (double)y, sum[2] += (double)z;
    }
  }
  if (bad) atomicOr(&sbad, 1);
  for (int d = 0; d < 3; ++d) {
    const double w = wave_sum_d(sum[d]);
    if ((threadIdx.x & 63) == 0) ssum[d][threadIdx.x >> 6] = w;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double P[12], G[12];
  bool pbad = sbad != 0;
  for (int k = 0; k < 12; ++k) {
    G[k] = (double)pose[12 * (size_t)b + k];
    P[k] = mode == SPR_AUG_NONE ? ((k % 5 == 0) ? 1.0 : 0.0) : (double)perturb[12 * (size_t)b + k];
    pbad = pbad || !aug_finite((float)G[k]) || !aug_finite((float)P[k]);
  }
  if (mode == SPR_AUG_SMALL) {
    const int n = pside ? tgt_cu[b + 1] - tgt_cu[b] : src_cu[b + 1] - src_cu[b];
    double c[3];
    for (int d = 0; d < 3; ++d) {
      double s = 0.0;
      for (int w = 0; w < (int)(blockDim.x >> 6); ++w) s += ssum[d][w];
      c[d] = n > 0 ? (double)(float)(s / (double)n) : 0.0;
    }
    for (int k = 0; k < 3; ++k)
      P[4 * k + 3] = __dadd_rn(aug_dot3(P[4 * k], -c[0], P[4 * k + 1], -c[1], P[4 * k + 2], -c[2]),
                               __dadd_rn(P[4 * k + 3], c[k]));
    aug_round(P);
  }
  double Q[12], I[12];
  if (mode == SPR_AUG_NONE) {
    for (int k = 0; k < 12; ++k) Q[k] = G[k];
  } else if (pside == 0) {
    aug_inv(P, I);
    aug_cat(G, I, Q);
  } else {
    aug_cat(P, G, Q);
  }
  aug_round(Q);
  if (f & 2) {
    aug_inv(Q, I);
    aug_round(I);
    for (int k = 0; k < 12; ++k) Q[k] = I[k];
  }
  for (int k = 0; k < 12; ++k) {
    T[12 * (size_t)b + k] = (float)P[k];
    out_pose[12 * (size_t)b + k] = (float)Q[k];
  }
  status[b] = pbad ? 1 : 0;
}

// Thread p owns position p of the sorted order: rank p - beg of cloud c's permutation.
__global__ __launch_bounds__(256) void k_aug_gather(
    int np, int ns, int nb, const unsigned long long* __restrict__ skey, const unsigned int* __restrict__ sval,
    const float* __restrict__ src_xyz, const int* __restrict__ src_cu, const float* __restrict__ tgt_xyz,
    const int* __restrict__ tgt_cu, const unsigned char* __restrict__ src_mask,
    const unsigned char* __restrict__ tgt_mask, int has_mask, const unsigned char* __restrict__ flags, int mode,
    float scale, int max_pts, uint64_t seed, const uint64_t* __restrict__ pair_key, const float* __restrict__ noise,
    const float* __restrict__ T, const int* __restrict__ out_src_cu, const int* __restrict__ out_tgt_cu,
    int* __restrict__ inv, float* __restrict__ out_src_xyz, float* __restrict__ out_tgt_xyz,
    unsigned char* __restrict__ out_src_mask, unsigned char* __restrict__ out_tgt_mask,
    int* __restrict__ out_src_perm, int* __restrict__ out_tgt_perm) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= np) return;
  const int c = (int)(skey[p] >> 32);
  const int g = (int)sval[p];
  if (c < 0 || c >= 2 * nb || g < 0 || g >= np) return;  // not reachable: both come from k_aug_keys
  const AugCloud a = aug_cloud(c, nb, ns, src_cu, tgt_cu);
  const int r = p - a.beg, i = g - a.beg;
  if (r < 0 || r >= a.len || i < 0 || i >= a.len) return;
  const bool keep = r < max_pts;
  inv[g] = keep ? r : -1;
  if (!keep) return;
  const int f = flags[a.pair];
  const float* in = a.side ? tgt_xyz + 3 * (size_t)(g - ns) : src_xyz + 3 * (size_t)g;
  float x = in[0], y = in[1], z = in[2];
  if (mode != SPR_AUG_NONE && a.side == ((f & 1) ? 0 : 1)) {
    const float* t = T + 12 * (size_t)a.pair;
    const double xd = (double)x, yd = (double)y, zd = (double)z;
    x = (float)__dadd_rn(aug_dot3((double)t[0], xd, (double)t[1], yd, (double)t[2], zd), (double)t[3]);
    y = (float)__dadd_rn(aug_dot3((double)t[4], xd, (double)t[5], yd, (double)t[6], zd), (double)t[7]);
    z = (float)__dadd_rn(aug_dot3((double)t[8], xd, (double)t[9], yd, (double)t[10], zd), (double)t[11]);
  }
  float n[3];
  if (noise) {
    n[0] = noise[3 * (size_t)g], n[1] = noise[3 * (size_t)g + 1], n[2] = noise[3 * (size_t)g + 2];
  } else {
    aug_noise(seed, pair_key[a.pair], a.side, i, n);
  }
  x = __fadd_rn(x, __fmul_rn(n[0], scale));
  y = __fadd_rn(y, __fmul_rn(n[1], scale));
  z = __fadd_rn(z, __fmul_rn(n[2], scale));
  const int oside = a.side ^ ((f >> 1) & 1);
  const size_t o = (size_t)(oside ? out_tgt_cu : out_src_cu)[a.pair] + (size_t)r;
  float* out = (oside ? out_tgt_xyz : out_src_xyz) + 3 * o;
  out[0] = x, out[1] = y, out[2] = z;
  (oside ? out_tgt_perm : out_src_perm)[o] = i;
  if (has_mask) (oside ? out_tgt_mask : out_src_mask)[o] = a.side ? tgt_mask[g - ns] : src_mask[g];
}

// the pair owning column j of the correspondence array, -1 if none; its run as (off, cnt) clamped into the array
__device__ __forceinline__ int2 aug_corr_run(int c, int stride, const int* __restrict__ off,
                                             const int* __restrict__ cnt) {
  const int o = off[c];
  if (o < 0 || o > stride) return make_int2(0, 0);
  return make_int2(o, max(0, min(cnt[c], stride - o)));
}
__device__ __forceinline__ int aug_corr_pair(int j, int nb, int stride, const int* __restrict__ off,
                                             const int* __restrict__ cnt) {
  if (nb <= 0 || off[0] > j) return -1;
  int lo = 0, hi = nb;  // off[lo] <= j < off[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] <= j)
      lo = mid;
    else
      hi = mid;
  }
  const int2 run = aug_corr_run(lo, stride, off, cnt);
  return (j >= run.x && j < run.x + run.y) ? lo : -1;
}

// flag[j] = column j holds a correspondence whose two ends survive; ra / rb = its ends' new indices; flag[stride] = 0
__global__ __launch_bounds__(256) void k_aug_cmark(int stride, int ns, int nb, const int* __restrict__ corr,
                                                   const int* __restrict__ off, const int* __restrict__ cnt,
                                                   const int* __restrict__ src_cu, const int* __restrict__ tgt_cu,
                                                   const int* __restrict__ inv, int* __restrict__ flag,
                                                   int* __restrict__ ra, int* __restrict__ rb) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j > stride) return;
  int f = 0;
  if (j < stride) {
    const int c = aug_corr_pair(j, nb, stride, off, cnt);
    if (c >= 0) {
      const int a = corr[j], b = corr[(size_t)stride + j];
      if (a >= 0 && a < src_cu[c + 1] - src_cu[c] && b >= 0 && b < tgt_cu[c + 1] - tgt_cu[c]) {
        const int na = inv[src_cu[c] + a], nbi = inv[ns + tgt_cu[c] + b];
        ra[j] = na;
        rb[j] = nbi;
        f = (na >= 0 && nbi >= 0) ? 1 : 0;
      }
    }
  }
  flag[j] = f;
}

__global__ __launch_bounds__(256) void k_aug_ccompact(int stride, int nb, const int* __restrict__ off,
                                                      const int* __restrict__ cnt,
                                                      const unsigned char* __restrict__ flags,
                                                      const int* __restrict__ flag, const int* __restrict__ pos,
                                                      const int* __restrict__ ra, const int* __restrict__ rb,
                                                      int* __restrict__ out_corr, int* __restrict__ out_count) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < nb) {
    const int2 run = aug_corr_run(j, stride, off, cnt);
    out_count[j] = pos[run.x + run.y] - pos[run.x];
  }
  if (j >= stride || !flag[j]) return;
  const int c = aug_corr_pair(j, nb, stride, off, cnt);
  if (c < 0) return;
  const int2 run = aug_corr_run(c, stride, off, cnt);
  const int o = run.x + (pos[j] - pos[run.x]);
  const bool swap = (flags[c] & 2) != 0;
  out_corr[o] = swap ? rb[j] : ra[j];
  out_corr[(size_t)stride + o] = swap ? ra[j] : rb[j];
}

int aug_sort_bits(int nb) {
  int bits = 33;
  while (bits < 48 && (1ull << (bits - 32)) < 2ull * (unsigned long long)nb) ++bits;
  return bits;
}

size_t aug_temp_bytes(size_t np, size_t stride, int nb) {
  size_t a = 0, b = 0;
  (void)rocprim::radix_sort_pairs(nullptr, a, (unsigned long long*)nullptr, (unsigned long long*)nullptr,
                                  (unsigned int*)nullptr, (unsigned int*)nullptr, (unsigned int)(np > 0 ? np : 1), 0,
                                  aug_sort_bits(nb));
  (void)rocprim::exclusive_scan(nullptr, b, (int*)nullptr, (int*)nullptr, 0, stride + 1, rocprim::plus<int>());
  return align_up(a > b ? a : b, 256) + 256;
}

// No points are measured as one point, no pairs as one pair (the size query's clamp).
struct AugWs {
  unsigned long long *skey, *skey2;   // sort keys in / out
  unsigned int *sval, *sval2;         // sort values in / out
  int* inv;                           // inverse permutation
  float* T;                           // P' per pair
  int *flag, *pos, *ra, *rb;          // survivor flags, their prefix, remapped ends
  size_t temp_bytes;
  void* temp;
};
AugWs aug_layout(Workspace& w, int ns, int nt, int nb, int stride) {
  const size_t np = (size_t)ns + (size_t)nt, P = np > 0 ? np : 1, S = (size_t)stride;
  AugWs l;
  l.skey = w.take<unsigned long long>(P);
  l.skey2 = w.take<unsigned long long>(P);
  l.sval = w.take<unsigned int>(P);
  l.sval2 = w.take<unsigned int>(P);
  l.inv = w.take<int>(P);
  l.T = w.take<float>(12 * (size_t)(nb > 0 ? nb : 1));
  l.flag = w.take<int>(S + 1);
  l.pos = w.take<int>(S + 1);
  l.ra = w.take<int>(S + 1);
  l.rb = w.take<int>(S + 1);
  l.temp_bytes = aug_temp_bytes(P, S, nb);
  l.temp = w.take<char>(l.temp_bytes);
  return l;
}

// ---- pair decisions: float64 on the host -------------------------------------------------------------------------
double aug_u64(uint32_t w) { return ((double)(w >> 9) + 0.5) * 1.1920928955078125e-7; }
constexpr double kAugPi = 3.14159265358979323846;

void aug_normal2(uint32_t a, uint32_t b, double* c, double* s) {
  const double r = std::sqrt(-2.0 * std::log(aug_u64(a))), t = 2.0 * kAugPi * aug_u64(b);
  *c = r * std::cos(t);
  *s = r * std::sin(t);
}

void aug_decide(uint64_t seed, uint64_t pair_key, int mode, unsigned char* perturb_src, unsigned char* swap,
                float* P) {
  const Philox4 b0 = philox_block(seed, pair_key, 0, 0, kTagPair);
  if (perturb_src) *perturb_src = aug_u64(b0.w[0]) > 0.5 ? 1 : 0;
  if (swap) *swap = aug_u64(b0.w[1]) > 0.5 ? 1 : 0;
  if (!P) return;
  double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, 0};
  if (mode != SPR_AUG_NONE) {
    const Philox4 b1 = philox_block(seed, pair_key, 0, 1, kTagPair), b2 = philox_block(seed, pair_key, 0, 2, kTagPair);
    if (mode == SPR_AUG_SMALL) {
      const double std_ = 0.1;
      const double z = 2.0 * aug_u64(b1.w[0]) - 1.0, s = std::sqrt(1.0 - z * z), phi = 2.0 * kAugPi * aug_u64(b1.w[1]);
      const double k[3] = {s * std::cos(phi), s * std::sin(phi), z};
      double nc, nsn;
      aug_normal2(b1.w[2], b1.w[3], &nc, &nsn);
      const double th = nc * std_ * kAugPi / std::sqrt(3.0), ct = std::cos(th), st = std::sin(th), vt = 1.0 - ct;
      const double K[9] = {0, -k[2], k[1], k[2], 0, -k[0], -k[1], k[0], 0};
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R[3 * i + j] = (i == j ? ct : 0.0) + st * K[3 * i + j] + vt * k[i] * k[j];
      double t0, t1, t2, unused;
      aug_normal2(b2.w[0], b2.w[1], &t0, &t1);
      aug_normal2(b2.w[2], b2.w[3], &t2, &unused);
      const double f = std_ / std::sqrt(3.0);
      t[0] = t0 * f, t[1] = t1 * f, t[2] = t2 * f;
    } else {
      const double az = 2.0 * kAugPi * aug_u64(b1.w[0]), ay = 2.0 * kAugPi * aug_u64(b1.w[1]),
                   ax = 2.0 * kAugPi * aug_u64(b1.w[2]);
      const double cz = std::cos(az), sz = std::sin(az), cy = std::cos(ay), sy = std::sin(ay), cx = std::cos(ax),
                   sx = std::sin(ax);
      // extrinsic z, then y, then x: R = Rx Ry Rz
      const double Rz[9] = {cz, -sz, 0, sz, cz, 0, 0, 0, 1}, Ry[9] = {cy, 0, sy, 0, 1, 0, -sy, 0, cy},
                   Rx[9] = {1, 0, 0, 0, cx, -sx, 0, sx, cx};
      double A[9];
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) A[3 * i + j] = Ry[3 * i] * Rz[j] + Ry[3 * i + 1] * Rz[3 + j] + Ry[3 * i + 2] * Rz[6 + j];
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R[3 * i + j] = Rx[3 * i] * A[j] + Rx[3 * i + 1] * A[3 + j] + Rx[3 * i + 2] * A[6 + j];
      for (int d = 0; d < 3; ++d) t[d] = -4.0 + 8.0 * aug_u64(b2.w[d]);
    }
  }
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) P[4 * i + j] = (float)R[3 * i + j];
    P[4 * i + 3] = (float)t[i];
  }
}

}  // namespace
}  // namespace spr

using namespace spr;

extern "C" int spr_philox4x32_host(const uint32_t* ctr_host, const uint32_t* key_host, uint32_t* out_host) {
  SPR_REQUIRE(ctr_host && key_host && out_host, "philox4x32_host: null pointer");
  const Philox4 o = philox4x32_10(ctr_host[0], ctr_host[1], ctr_host[2], ctr_host[3], key_host[0], key_host[1]);
  for (int k = 0; k < 4; ++k) out_host[k] = o.w[k];
  return 0;
}

extern "C" int spr_augment_draw(uint64_t seed, const uint64_t* pair_key_host, int nb, int mode,
                                unsigned char* perturb_src_host, unsigned char* swap_host, float* perturb_host,
                                const uint64_t* pair_key, const int* src_cu, int ns, const int* tgt_cu, int nt,
                                float* noise, unsigned int* keys, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPR_REQUIRE(nb >= 0 && ns >= 0 && nt >= 0, "augment_draw: negative size (nb=%d ns=%d nt=%d)", nb, ns, nt);
  SPR_REQUIRE(mode == SPR_AUG_NONE || mode == SPR_AUG_SMALL || mode == SPR_AUG_LARGE, "augment_draw: unknown mode %d", mode);
  if (perturb_src_host || swap_host || perturb_host) {
    SPR_REQUIRE(nb == 0 || pair_key_host, "augment_draw: pair_key_host must not be null");
    for (int b = 0; b < nb; ++b) {
      SPR_REQUIRE(pair_key_host[b] < (1ull << 63), "augment_draw: pair_key[%d] must be below 2^63", b);
      aug_decide(seed, pair_key_host[b], mode, perturb_src_host ? perturb_src_host + b : nullptr,
                 swap_host ? swap_host + b : nullptr, perturb_host ? perturb_host + 12 * (size_t)b : nullptr);
    }
  }
  if (!noise && !keys) return 0;
  SPR_REQUIRE(nb < 32768, "augment_draw: at most 32767 pairs per call");
  SPR_REQUIRE((size_t)ns + (size_t)nt <= ((size_t)1 << 26), "augment_draw: at most 2^26 points per call");
  SPR_REQUIRE(nb > 0 || (ns == 0 && nt == 0), "augment_draw: points without pairs (nb=0 ns=%d nt=%d)", ns, nt);
  const int np = ns + nt;
  if (np == 0) return 0;
  SPR_REQUIRE(pair_key && src_cu && tgt_cu, "augment_draw: pair_key, src_cu and tgt_cu (device) must not be null");
  hipLaunchKernelGGL(k_aug_draw, dim3(cdiv(np, 256)), dim3(256), 0, stream, np, ns, nb, src_cu, tgt_cu, seed, pair_key,
                     noise, keys);
  SPR_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t spr_augment_workspace_bytes(int ns, int nt, int nb, int corr_stride) {
  if (ns < 0 || nt < 0 || nb < 0 || corr_stride < 0) return 0;
  return measure(aug_layout, ns, nt, nb, corr_stride);
}

extern "C" int spr_augment_pairs(const float* src_xyz, const int* src_cu, int ns, const float* tgt_xyz,
                                 const int* tgt_cu, int nt, const float* pose, int nb, const unsigned char* src_mask,
                                 const unsigned char* tgt_mask, const int* corr, int corr_stride, const int* corr_off,
                                 const int* corr_count, const float* perturb, const unsigned char* flags, int mode,
                                 float scale, int max_pts, uint64_t seed, const uint64_t* pair_key, const float* noise,
                                 const unsigned int* keys, float* out_src_xyz, float* out_tgt_xyz, int* out_src_cu,
                                 int* out_tgt_cu, float* out_pose, unsigned char* out_src_mask,
                                 unsigned char* out_tgt_mask, int* out_src_perm, int* out_tgt_perm, int* out_corr,
                                 int* out_corr_count, int* status, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPR_REQUIRE(nb >= 0 && ns >= 0 && nt >= 0, "augment_pairs: negative size (nb=%d ns=%d nt=%d)", nb, ns, nt);
  SPR_REQUIRE(mode == SPR_AUG_NONE || mode == SPR_AUG_SMALL || mode == SPR_AUG_LARGE, "augment_pairs: unknown mode %d", mode);
  SPR_REQUIRE(max_pts >= 1, "augment_pairs: max_pts must be at least 1, got %d", max_pts);
  SPR_REQUIRE(scale >= 0.f && scale < 3.0e38f, "augment_pairs: scale must be finite and >= 0");
  SPR_REQUIRE(nb < 32768, "augment_pairs: at most 32767 pairs per call");
  SPR_REQUIRE((size_t)ns + (size_t)nt <= ((size_t)1 << 26), "augment_pairs: at most 2^26 points per call");
  SPR_REQUIRE(nb > 0 || (ns == 0 && nt == 0), "augment_pairs: points without pairs (nb=0 ns=%d nt=%d)", ns, nt);
  if (nb == 0) return 0;
  SPR_REQUIRE(src_cu && tgt_cu && pose && flags && out_src_cu && out_tgt_cu && out_pose && status,
              "augment_pairs: src_cu, tgt_cu, pose, flags, out_src_cu, out_tgt_cu, out_pose and status must not be null");
  SPR_REQUIRE(mode == SPR_AUG_NONE || perturb, "augment_pairs: perturb must not be null unless mode is SPR_AUG_NONE");
  SPR_REQUIRE(ns == 0 || src_xyz, "augment_pairs: null source pointer with ns=%d", ns);
  SPR_REQUIRE(nt == 0 || tgt_xyz, "augment_pairs: null target pointer with nt=%d", nt);
  const int np = ns + nt;
  SPR_REQUIRE(np == 0 || (out_src_xyz && out_tgt_xyz && out_src_perm && out_tgt_perm),
              "augment_pairs: null output pointer");
  const bool masks = src_mask || tgt_mask;
  SPR_REQUIRE(!masks || ((ns == 0 || src_mask) && (nt == 0 || tgt_mask) && out_src_mask && out_tgt_mask),
              "augment_pairs: masks come for both clouds, with both outputs, or not at all");
  SPR_REQUIRE((keys && noise) || pair_key, "augment_pairs: pair_key must not be null when noise or keys are generated inline");
  SPR_REQUIRE(corr_stride >= 0, "augment_pairs: negative corr_stride");
  SPR_REQUIRE(!corr || (corr_off && corr_count && out_corr_count && (corr_stride == 0 || out_corr)),
              "augment_pairs: corr needs corr_off, corr_count, out_corr and out_corr_count");
  const int stride = corr ? corr_stride : 0;
  Workspace w(ws, ws_bytes);
  const auto [skey, skey2, sval, sval2, inv, T, flag, pos, ra, rb, temp_bytes, temp] = aug_layout(w, ns, nt, nb, stride);
  SPR_REQUIRE(ws != nullptr && w.ok(), "augment_pairs: workspace too small");

  const int TB = 256;
  hipLaunchKernelGGL(k_aug_layout, dim3(1), dim3(64), 0, stream, nb, max_pts, src_cu, tgt_cu, flags, out_src_cu,
                     out_tgt_cu);
  hipLaunchKernelGGL(k_aug_pose, dim3(nb), dim3(1024), 0, stream, nb, ns, src_xyz, src_cu, tgt_xyz, tgt_cu, pose, perturb,
                     flags, mode, T, out_pose, status);
  SPR_LAUNCH_CHECK();
  if (np > 0) {
    hipLaunchKernelGGL(k_aug_keys, dim3(cdiv(np, TB)), dim3(TB), 0, stream, np, ns, nb, src_cu, tgt_cu, seed, pair_key,
                       keys, skey, sval);
    SPR_LAUNCH_CHECK();
    size_t tb = temp_bytes;
    SPR_HIP_CHECK(rocprim::radix_sort_pairs(temp, tb, skey, skey2, sval, sval2, (unsigned int)np, 0, aug_sort_bits(nb),
                                            stream));
    hipLaunchKernelGGL(k_aug_gather, dim3(cdiv(np, TB)), dim3(TB), 0, stream, np, ns, nb, skey2, sval2, src_xyz, src_cu,
                       tgt_xyz, tgt_cu, src_mask, tgt_mask, masks ? 1 : 0, flags, mode, scale, max_pts, seed, pair_key, noise, T,
                       out_src_cu, out_tgt_cu, inv, out_src_xyz, out_tgt_xyz, out_src_mask, out_tgt_mask, out_src_perm,
                       out_tgt_perm);
    SPR_LAUNCH_CHECK();
  }
  if (corr) {
    hipLaunchKernelGGL(k_aug_cmark, dim3(cdiv(stride + 1, TB)), dim3(TB), 0, stream, stride, ns, nb, corr, corr_off,
                       corr_count, src_cu, tgt_cu, inv, flag, ra, rb);
    SPR_LAUNCH_CHECK();
    size_t tb = temp_bytes;
    SPR_HIP_CHECK(rocprim::exclusive_scan(temp, tb, flag, pos, 0, (size_t)stride + 1, rocprim::plus<int>(), stream));
    hipLaunchKernelGGL(k_aug_ccompact, dim3(cdiv(stride > nb ? stride : nb, TB)), dim3(TB), 0, stream, stride, nb,
                       corr_off, corr_count, flags, flag, pos, ra, rb, out_corr, out_corr_count);
    SPR_LAUNCH_CHECK();
  }
  return 0;
}
