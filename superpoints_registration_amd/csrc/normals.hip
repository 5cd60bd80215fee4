// Surface normals as per-point input features (include/spr.h, "surface normals"): spr_estimate_normals and
// spr_feats_gather_rotate.
//
// k_normals.  A gather-bound kernel: per point one row of kmax int32 indices and kmax 12-byte point gathers, then a
// few hundred flops.  kGroup = 8 lanes share a point (8 points per wave, 32 per block): lane g of the group reads
// columns g, g + 8, ... of the row, so the group's index loads are 32-byte runs, and a step issues kStep index loads
// and then kStep point gathers per lane before any of them is consumed.  Every lane accumulates the count and the
// nine moments of d = p_j - p_i (sum d: 3, sum d d^T: 6) over its columns in column order; a three-step xor butterfly
// inside the group leaves the same sums in all eight lanes (float addition commutes, so both partners of a step get
// the same bits).  Moments relative to the query point: a cloud at KITTI coordinates is as well conditioned as one at
// the origin.  The 3x3 eigenproblem is solved redundantly by every lane of the group, in registers: cyclic Jacobi on
// the covariance divided by its trace.  Lanes 0..2 of a group store one component each (a wave writes 96 contiguous
// bytes).  No LDS, no atomics, no workspace; results do not depend on the launch geometry.
//
// k_gather_rotate.  One thread per output element; a column inside a listed triple reads its triple and applies row
// k of the cloud's rotation in float64 (one rounding per operation, then one to float32), every other column is a
// copy.  The cloud of a row comes from a binary search in cu_out.
#include "spr_common.h"

namespace spr {
namespace {

constexpr int kGroup = 8;     // lanes per point
constexpr int kStep = 4;      // neighbour columns a lane has in flight
constexpr int kBlock = 256;   // 32 points per workgroup
constexpr int kSweeps = 8;    // cyclic Jacobi, 3x3 float32: converged after 4 to 5
constexpr int kMaxTriples = 4;

struct Triples {
  int n;
  int col[kMaxTriples];
};

// One Jacobi rotation in the (p, q) plane of a symmetric 3x3: app, aqq, apq and the two entries arp, arq that couple
// p and q to the third index r; vp, vq are columns p and q of the accumulated eigenvector matrix.
__device__ __forceinline__ void jacobi_rotate(float& app, float& aqq, float& apq, float& arp, float& arq, float (&vp)[3],
                                              float (&vq)[3]) {
  if (apq == 0.f) return;
  const float theta = (aqq - app) / (2.f * apq);             // |theta| may overflow to inf: t = 0, a no-op
  const float t = (theta >= 0.f ? 1.f : -1.f) / (fabsf(theta) + sqrtf(theta * theta + 1.f));
  const float c = 1.f / sqrtf(t * t + 1.f), s = t * c;
  app -= t * apq;
  aqq += t * apq;
  apq = 0.f;
  const float rp = arp, rq = arq;
  arp = c * rp - s * rq;
  arq = s * rp + c * rq;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float a = vp[k], b = vq[k];
    vp[k] = c * a - s * b;
    vq[k] = s * a + c * b;
  }
}

__global__ __launch_bounds__(kBlock) void k_normals(const float* __restrict__ xyz, const int* __restrict__ cu, int n,
                                                    int nb, const int* __restrict__ nbr, int nbr_stride, int kmax,
                                                    const float* __restrict__ viewpoint, float* __restrict__ normals,
                                                    float* __restrict__ curvature) {
  const int g = threadIdx.x & (kGroup - 1);
  const long pt = (long)blockIdx.x * (kBlock / kGroup) + (threadIdx.x / kGroup);
  const bool live = pt < n;                     // a whole group is live or not: its shuffles stay inside the group
  const int i = live ? (int)pt : 0;
  float px = 0.f, py = 0.f, pz = 0.f;
  if (live) {
    px = xyz[3 * (size_t)i];
    py = xyz[3 * (size_t)i + 1];
    pz = xyz[3 * (size_t)i + 2];
  }
  float cnt = 0.f, sx = 0.f, sy = 0.f, sz = 0.f, sxx = 0.f, sxy = 0.f, sxz = 0.f, syy = 0.f, syz = 0.f, szz = 0.f;
  if (live) {
    const int* row = nbr + (size_t)i * nbr_stride;
    for (int c0 = g; c0 < kmax; c0 += kGroup * kStep) {
      int idx[kStep];
      float qx[kStep], qy[kStep], qz[kStep];
#pragma unroll
      for (int u = 0; u < kStep; ++u) {
        const int col = c0 + u * kGroup;
        idx[u] = col < kmax ? row[col] : -1;
      }
#pragma unroll
      for (int u = 0; u < kStep; ++u) {
        const bool ok = (unsigned)idx[u] < (unsigned)n;     // anything outside [0, n) is a shadow
        const size_t j = ok ? (size_t)idx[u] : (size_t)i;
        qx[u] = xyz[3 * j];
        qy[u] = xyz[3 * j + 1];
        qz[u] = xyz[3 * j + 2];
      }
#pragma unroll
      for (int u = 0; u < kStep; ++u) {
        if ((unsigned)idx[u] < (unsigned)n) {
          const float dx = qx[u] - px, dy = qy[u] - py, dz = qz[u] - pz;
          cnt += 1.f;
          sx += dx;
          sy += dy;
          sz += dz;
          sxx += dx * dx;
          sxy += dx * dy;
          sxz += dx * dz;
          syy += dy * dy;
          syz += dy * dz;
          szz += dz * dz;
        }
      }
    }
  }
#pragma unroll
  for (int o = 1; o < kGroup; o <<= 1) {
    cnt += __shfl_xor(cnt, o, 64);
    sx += __shfl_xor(sx, o, 64);
    sy += __shfl_xor(sy, o, 64);
    sz += __shfl_xor(sz, o, 64);
    sxx += __shfl_xor(sxx, o, 64);
    sxy += __shfl_xor(sxy, o, 64);
    sxz += __shfl_xor(sxz, o, 64);
    syy += __shfl_xor(syy, o, 64);
    syz += __shfl_xor(syz, o, 64);
    szz += __shfl_xor(szz, o, 64);
  }
  if (!live || g >= 3) return;

  float nrm[3] = {0.f, 0.f, 0.f};
  float curv = 0.f;
  if (cnt >= 3.f) {
    const float inv = 1.f / cnt;
    const float mx = sx * inv, my = sy * inv, mz = sz * inv;
    float a00 = sxx * inv - mx * mx, a01 = sxy * inv - mx * my, a02 = sxz * inv - mx * mz;
    float a11 = syy * inv - my * my, a12 = syz * inv - my * mz, a22 = szz * inv - mz * mz;
    const float tr = (a00 + a11) + a22;
    if (tr > 0.f) {                                // scale-free: the rotations see entries of magnitude <= 1
      const float s = 1.f / tr;
      a00 *= s, a01 *= s, a02 *= s, a11 *= s, a12 *= s, a22 *= s;
    }
    float v0[3] = {1.f, 0.f, 0.f}, v1[3] = {0.f, 1.f, 0.f}, v2[3] = {0.f, 0.f, 1.f};
    for (int sweep = 0; sweep < kSweeps; ++sweep) {
      if (a01 == 0.f && a02 == 0.f && a12 == 0.f) break;
      jacobi_rotate(a00, a11, a01, a02, a12, v0, v1);
      jacobi_rotate(a00, a22, a02, a01, a12, v0, v2);
      jacobi_rotate(a11, a22, a12, a01, a02, v1, v2);
    }
    // the smallest eigenvalue's column; among equal eigenvalues the lowest index
    float l0 = a00;
    float e[3] = {v0[0], v0[1], v0[2]};
    if (a11 < l0) {
      l0 = a11;
      e[0] = v1[0], e[1] = v1[1], e[2] = v1[2];
    }
    if (a22 < l0) {
      l0 = a22;
      e[0] = v2[0], e[1] = v2[1], e[2] = v2[2];
    }
    const float len = sqrtf((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
    e[0] /= len, e[1] /= len, e[2] /= len;
    const float sum = (a00 + a11) + a22;
    curv = tr > 0.f ? fmaxf(l0, 0.f) / sum : 0.f;

    // sign: towards the viewpoint of the point's cloud; without one, or on a product of exactly 0, the component of
    // largest magnitude is made positive (the lowest index among equal magnitudes)
    float side = 0.f;
    if (viewpoint != nullptr) {
      const int b = find_segment(cu, nb, i);
      const float wx = viewpoint[3 * b] - px, wy = viewpoint[3 * b + 1] - py, wz = viewpoint[3 * b + 2] - pz;
      side = (e[0] * wx + e[1] * wy) + e[2] * wz;
    }
    if (side == 0.f) {
      side = e[0];
      if (fabsf(e[1]) > fabsf(side)) side = e[1];
      if (fabsf(e[2]) > fabsf(side)) side = e[2];
    }
    const bool flip = side < 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) nrm[k] = flip ? -e[k] : e[k];
  }
  normals[3 * (size_t)i + g] = g == 0 ? nrm[0] : (g == 1 ? nrm[1] : nrm[2]);
  if (g == 0 && curvature != nullptr) curvature[i] = curv;
}

__global__ __launch_bounds__(kBlock) void k_gather_rotate(const float* __restrict__ feats, int n_in, int c,
                                                          const int* __restrict__ rows, long total,
                                                          const int* __restrict__ cu_out, int nb,
                                                          const float* __restrict__ rot, Triples tr,
                                                          float* __restrict__ out) {
  const long e = (long)blockIdx.x * kBlock + threadIdx.x;
  if (e >= total) return;
  const int r = (int)(e / c);
  const int col = (int)(e - (long)r * c);
  const int src = rows[r];
  float v = 0.f;                                  // a source row outside [0, n_in) reads zeros
  if ((unsigned)src < (unsigned)n_in) {
    const float* f = feats + (size_t)src * c;
    int k = -1, start = 0;
#pragma unroll
    for (int t = 0; t < kMaxTriples; ++t)
      if (t < tr.n && col >= tr.col[t] && col < tr.col[t] + 3) {
        k = col - tr.col[t];
        start = tr.col[t];
      }
    if (k < 0) {
      v = f[col];
    } else {
      const float* m = rot + 9 * (size_t)find_segment(cu_out, nb, r) + 3 * k;
      v = (float)(((double)m[0] * (double)f[start] + (double)m[1] * (double)f[start + 1]) +
                  (double)m[2] * (double)f[start + 2]);
    }
  }
  out[e] = v;
}

}  // namespace
}  // namespace spr

using namespace spr;

extern "C" int spr_estimate_normals(const float* xyz, const int* cu, int n, int nb, const int* nbr, int nbr_stride,
                                    int kmax, const float* viewpoint, float* normals, float* curvature,
                                    void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPR_REQUIRE(n >= 0 && nb >= 0 && kmax >= 0 && nbr_stride >= kmax,
              "estimate_normals: bad arguments (n %d, nb %d, kmax %d, nbr_stride %d)", n, nb, kmax, nbr_stride);
  if (n == 0) return 0;
  SPR_REQUIRE(xyz != nullptr && normals != nullptr && (nbr != nullptr || kmax == 0),
              "estimate_normals: null pointer");
  SPR_REQUIRE(viewpoint == nullptr || (cu != nullptr && nb >= 1),
              "estimate_normals: a viewpoint per cloud needs cu and nb >= 1");
  const int per_block = kBlock / kGroup;
  hipLaunchKernelGGL(k_normals, dim3((unsigned)cdiv(n, per_block)), dim3(kBlock), 0, stream, xyz, cu, n, nb, nbr,
                     nbr_stride, kmax, viewpoint, normals, curvature);
  SPR_LAUNCH_CHECK();
  return 0;
}

extern "C" int spr_feats_gather_rotate(const float* feats, int n_in, int c, const int* rows, int n_out,
                                       const int* cu_out, int nb, const float* rot, const int* dir_cols_host,
                                       int n_dir, float* out, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPR_REQUIRE(n_in >= 0 && n_out >= 0 && c >= 1 && nb >= 0 && n_dir >= 0 && n_dir <= kMaxTriples,
              "feats_gather_rotate: bad arguments (n_in %d, n_out %d, c %d, nb %d, %d direction triples; at most %d)",
              n_in, n_out, c, nb, n_dir, kMaxTriples);
  SPR_REQUIRE(n_dir == 0 || dir_cols_host != nullptr, "feats_gather_rotate: null dir_cols_host");
  Triples tr;
  tr.n = n_dir;
  for (int t = 0; t < kMaxTriples; ++t) tr.col[t] = t < n_dir ? dir_cols_host[t] : -8;
  for (int t = 0; t < n_dir; ++t) {
    SPR_REQUIRE(tr.col[t] >= 0 && tr.col[t] + 3 <= c,
                "feats_gather_rotate: the triple at column %d runs past the %d columns", tr.col[t], c);
    for (int u = 0; u < t; ++u)
      SPR_REQUIRE(tr.col[t] - tr.col[u] >= 3 || tr.col[u] - tr.col[t] >= 3,
                  "feats_gather_rotate: the triples at columns %d and %d overlap", tr.col[u], tr.col[t]);
  }
  if (n_out == 0) return 0;
  SPR_REQUIRE(rows != nullptr && out != nullptr && (feats != nullptr || n_in == 0),
              "feats_gather_rotate: null pointer");
  SPR_REQUIRE(n_dir == 0 || (cu_out != nullptr && rot != nullptr && nb >= 1),
              "feats_gather_rotate: direction triples need cu_out, rot and nb >= 1");
  const long total = (long)n_out * c;
  SPR_REQUIRE(total / kBlock < (1L << 31) - 1, "feats_gather_rotate: %d rows of %d columns exceed the grid", n_out, c);
  hipLaunchKernelGGL(k_gather_rotate, dim3((unsigned)cdiv(total, kBlock)), dim3(kBlock), 0, stream, feats, n_in, c, rows,
                     total, cu_out, nb, rot, tr, out);
  SPR_LAUNCH_CHECK();
  return 0;
}
