// Weighted Procrustes / Kabsch for ONE point set by ONE 256-thread workgroup (compute_rigid_transform,
// utils/se3_torch.py:109-163): shared by spr_weighted_procrustes (match_pose.hip) and spr_refine_pairs (refine.hip), so
// both solve with the same arithmetic in the same order -- float64 accumulation, thread t sums points t, t + 256, ...,
// wave shuffles, then the four wave partials in order; 3x3 SVD by one-sided Jacobi on thread 0.
#pragma once
#include "spr_common.h"

namespace spr {
#ifdef __HIPCC__

static __device__ void block_reduce_d(double* vals, int nvals, double* sh /*[256]*/) {
  // reduces each of vals[0..nvals) over the 256 threads; result in all threads
  for (int k = 0; k < nvals; ++k) {
    double x = wave_sum_d(vals[k]);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = x;
    __syncthreads();
    vals[k] = sh[0] + sh[1] + sh[2] + sh[3];
  }
}

static __device__ void svd3_jacobi(const double A[3][3], double U[3][3], double S[3], double V[3][3]) {
  double G[3][3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      G[i][j] = A[i][j];
      V[i][j] = (i == j) ? 1.0 : 0.0;
    }
  for (int sweep = 0; sweep < 30; ++sweep) {
    double off = 0.0;
    for (int p = 0; p < 2; ++p)
      for (int q = p + 1; q < 3; ++q) {
        double al = 0, be = 0, ga = 0;
        for (int k = 0; k < 3; ++k) {
          al += G[k][p] * G[k][p];
          be += G[k][q] * G[k][q];
          ga += G[k][p] * G[k][q];
        }
        if (ga == 0.0 || fabs(ga) <= 1e-30 * sqrt(al * be)) continue;
        off = fmax(off, fabs(ga) / sqrt(al * be + 1e-300));
        const double zeta = (be - al) / (2.0 * ga);
        const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
        for (int k = 0; k < 3; ++k) {
          const double gp = G[k][p], gq = G[k][q];
          G[k][p] = c * gp - s * gq;
          G[k][q] = s * gp + c * gq;
          const double vp = V[k][p], vq = V[k][q];
          V[k][p] = c * vp - s * vq;
          V[k][q] = s * vp + c * vq;
        }
      }
    if (off < 1e-15) break;
  }
  for (int j = 0; j < 3; ++j) S[j] = sqrt(G[0][j] * G[0][j] + G[1][j] * G[1][j] + G[2][j] * G[2][j]);
  // sort descending (torch.svd order)
  int ord[3] = {0, 1, 2};
  for (int a = 0; a < 2; ++a)
    for (int b = a + 1; b < 3; ++b)
      if (S[ord[b]] > S[ord[a]]) {
        int t = ord[a];
        ord[a] = ord[b];
        ord[b] = t;
      }
  double Gs[3][3], Vs[3][3], Ss[3];
  for (int j = 0; j < 3; ++j) {
    Ss[j] = S[ord[j]];
    for (int i = 0; i < 3; ++i) {
      Gs[i][j] = G[i][ord[j]];
      Vs[i][j] = V[i][ord[j]];
    }
  }
  const double tiny = 1e-14 * (Ss[0] > 0 ? Ss[0] : 1.0);
  for (int j = 0; j < 3; ++j) {
    S[j] = Ss[j];
    for (int i = 0; i < 3; ++i) {
      V[i][j] = Vs[i][j];
      U[i][j] = Ss[j] > tiny ? Gs[i][j] / Ss[j] : 0.0;
    }
  }
  // complete U for (numerically) rank deficient input
  if (!(S[0] > tiny)) {
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) U[i][j] = (i == j) ? 1.0 : 0.0;
    return;
  }
  if (!(S[1] > tiny)) {
    // any unit vector orthogonal to u0
    int m = 0;
    if (fabs(U[1][0]) < fabs(U[m][0])) m = 1;
    if (fabs(U[2][0]) < fabs(U[m][0])) m = 2;
    double e[3] = {0, 0, 0};
    e[m] = 1.0;
    const double d = U[m][0];
    double n2 = 0;
    for (int i = 0; i < 3; ++i) {
      U[i][1] = e[i] - d * U[i][0];
      n2 += U[i][1] * U[i][1];
    }
    n2 = sqrt(n2);
    for (int i = 0; i < 3; ++i) U[i][1] /= n2;
  }
  if (!(S[2] > tiny)) {
    U[0][2] = U[1][0] * U[2][1] - U[2][0] * U[1][1];
    U[1][2] = U[2][0] * U[0][1] - U[0][0] * U[2][1];
    U[2][2] = U[0][0] * U[1][1] - U[1][0] * U[0][1];
  }
}

// The serial end of the solve, shared with ransac.hip and icp.hip: the pose [R | t] (12 values, row-major [3,4], rounded
// to float32 when T is float, kept in float64 when T is double) from the reduced covariance cov [3x3, row-major] and
// the weighted centroids ca, cb.
template <class T>
static __device__ void procrustes_pose(const double* cov, const double* ca, const double* cb, T* out) {
  double A[3][3], U[3][3], S[3], V[3][3];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) A[r][c] = cov[3 * r + c];
  svd3_jacobi(A, U, S, V);
  // R = V U^T, flip V[:,2] when det <= 0  (se3_torch.py:150-157)
  double R[3][3];
  for (int pass = 0; pass < 2; ++pass) {
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c)
        R[r][c] = V[r][0] * U[c][0] + V[r][1] * U[c][1] + V[r][2] * U[c][2];
    const double det = R[0][0] * (R[1][1] * R[2][2] - R[1][2] * R[2][1]) -
                       R[0][1] * (R[1][0] * R[2][2] - R[1][2] * R[2][0]) +
                       R[0][2] * (R[1][0] * R[2][1] - R[1][1] * R[2][0]);
    if (det > 0.0) break;
    for (int r = 0; r < 3; ++r) V[r][2] = -V[r][2];
  }
  for (int r = 0; r < 3; ++r) {
    double t = cb[r];
    for (int c = 0; c < 3; ++c) {
      out[4 * r + c] = (T)R[r][c];
      t -= R[r][c] * ca[c];
    }
    out[4 * r + 3] = (T)t;
  }
}

// The pose [R | t] (12 floats, row-major [3,4]) of the weighted point set (a_i, b_i, w_i), i in [0, n): thread 0 writes
// it to `out` (global or LDS; no barrier behind the store).  a(i, d) / b(i, d): coordinate d of point i as float;
// w(i): its weight as float, read only when `weighted`.  Every thread of the 256-thread workgroup must call this;
// sh: 256 doubles of LDS.
template <class FA, class FB, class FW>
__device__ __forceinline__ void procrustes_block(int n, bool weighted, FA a, FB b, FW w, double* sh, float* out) {
  double acc[7] = {0, 0, 0, 0, 0, 0, 0};  // sum w, sum w*a (3), sum w*b (3)
  for (int i = threadIdx.x; i < n; i += 256) {
    const double wi = weighted ? (double)w(i) : 1.0;
    acc[0] += wi;
    for (int d = 0; d < 3; ++d) {
      acc[1 + d] += wi * (double)a(i, d);
      acc[4 + d] += wi * (double)b(i, d);
    }
  }
  block_reduce_d(acc, 7, sh);
  // se3_torch.py:136-139: w~ = w / clamp_min(sum w, 1e-6); unweighted: mean
  double den = weighted ? fmax(acc[0], 1e-6) : fmax(acc[0], 1.0);
  double ca[3], cb[3];
  for (int d = 0; d < 3; ++d) {
    ca[d] = acc[1 + d] / den;
    cb[d] = acc[4 + d] / den;
  }
  double cov[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = threadIdx.x; i < n; i += 256) {
    const double wi = (weighted ? (double)w(i) : 1.0) / den;
    double da[3], db[3];
    for (int d = 0; d < 3; ++d) {
      da[d] = (double)a(i, d) - ca[d];
      db[d] = ((double)b(i, d) - cb[d]) * wi;
    }
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) cov[3 * r + c] += da[r] * db[c];
  }
  block_reduce_d(cov, 9, sh);
  if (threadIdx.x == 0) procrustes_pose(cov, ca, cb, out);
}

#endif
}  // namespace spr
