// Point-to-point ICP for all pairs of a batch in one call, and the evaluation of a pose (fitness, inlier RMSE) that
// is its first pass, on gfx950.
//
// Behaviour contract: the loop of Open3D's registration_icp with TransformationEstimationPointToPoint, as the
// reference's KITTI loader runs it on every ground-truth pose (data_loaders/kitti_pred.py:161-183), written out as a
// float64 definition in include/spr.h ("ICP for all pairs").  Open3D itself is absent: parity with it is unpinned
// (DESIGN section 3), the definition in spr.h is what the tests hold the kernels to.
//
// One call:
//   k_icp_setup    per pair: non-finite test of the pose, the source and the target; the target's float64 bounding
//                  box -> its grid (ov_grid.h: cell edge >= max_dist (1 + 2^-8), coarser when the box needs more than
//                  16 n + 4096 cells); state T = pose_init; a refused pair is finished here (status -1)
//   k_icp_offsets  prefix of the cell counts and of the pairs' association blocks
//   k_icp_count -> rocPRIM exclusive scan -> k_icp_scatter: the TARGET clouds' cell table, built ONCE per call
//   per pass, for every pair that has not converged:
//     k_icp_assoc  one thread per source point: transform by T, walk the 27-cell neighbourhood (nine record runs),
//                  keep (d2, j) in registers, write corr; per block 17 float64 partials: count, sum a, sum b,
//                  sum a b^T, sum d2 (a = the transformed source, b = its partner, both minus the grid's origin)
//     k_icp_solve  one wave per pair: the partials reduced in a fixed order, fitness and RMSE, the convergence test,
//                  the Kabsch solve (procrustes_solve.h, float64 throughout), T <- U o T, or the pair's outputs
// One pass over the correspondences serves the evaluation of T_k and the solve for T_{k+1}: a pair that stops after
// `iterations` steps has cost iterations + 1 association passes.  A finished pair is frozen: its blocks leave at
// once, nothing of it is written again.  The host enqueues passes in chunks and reads ONE integer (the number of
// finished pairs) per chunk; since finished pairs are frozen the results do not depend on the chunk size.
//
// Order of the sums: block b of a pair holds its source points [256 b, 256 b + 256); inside a block wave shuffles
// (xor 32 .. 1), then the four waves in ascending order; the solve adds the blocks' partials lane-strided (lane l
// takes blocks l, l + 64, ..), then wave shuffles.  All of it is a function of the pair alone -- no floating-point
// atomics -- so every output of a pair has the same bits whatever batch it is called in, and run to run.  The order
// of the records inside a cell depends on integer-atomic arrival order; the minimum over (d2, index) does not.
//
// Point-to-plane ICP (spr_icp_plane_pairs; contract: spr.h, "Point-to-plane ICP for all pairs") is the same call with
// two other kernels in the pass: the setup, the cell table, the frozen pairs and the chunked read-back are shared.
//   k_icp_assoc_plane  the same walk; per block 29 float64 partials: count, sum d2, the 21 entries of the upper
//                      triangle of A = sum w J J^T and the 6 of g = sum w J r, J = [(a - c) x n ; n], c = the grid's
//                      origin (the target's per-axis minimum), w the robust kernel's weight of r
//   k_icp_solve_plane  the partials reduced in the same order, the same stopping rule, then in lane 0 the unpivoted
//                      LDL^T of A x = -g, the Euler composition of Open3D's TransformVector6dToMatrix4d and T <- U o T
#include "ov_grid.h"
#include "procrustes_solve.h"

namespace spr {
namespace {

constexpr int kIcpBlock = 256;
constexpr int kIcpParts = 17;   // count, sum a (3), sum b (3), sum a b^T (9), sum d2
constexpr int kIcpPlaneParts = 29;  // count, sum d2, upper triangle of sum w J J^T (21, row-major), sum w J r (6)
constexpr int kIcpChunk = 4;    // passes enqueued between two reads of the finished-pairs counter

__device__ __forceinline__ bool icp_finite(double v) { return fabs(v) < 1.0e300; }

__global__ __launch_bounds__(256) void k_icp_setup(const float* __restrict__ src, const int* __restrict__ src_cu,
                                                   const float* __restrict__ tgt, const int* __restrict__ tgt_cu,
                                                   const float* __restrict__ tgt_nrm,  // or null: no normals to test
                                                   const double* __restrict__ pose_init, double h0, OvGrid* info,
                                                   double* T, double* prev, int* iters, int* done, int* ndone,
                                                   float* pose, double* pose64, double* fitness, double* rmse,
                                                   int* iterations, int* count, int* corr, int* status) {
  const int c = blockIdx.x;
  const int sb = src_cu[c], se = src_cu[c + 1], tb = tgt_cu[c], te = tgt_cu[c + 1];
  __shared__ double smn[3][256], smx[3][256];
  __shared__ int sbad;
  if (threadIdx.x == 0) sbad = 0;
  __syncthreads();
  double mn[3] = {1.0e300, 1.0e300, 1.0e300}, mx[3] = {-1.0e300, -1.0e300, -1.0e300};
  bool bad = false;
  if (threadIdx.x < 12) bad = !icp_finite(pose_init[12 * (size_t)c + threadIdx.x]);
  for (int p = sb + threadIdx.x; p < se; p += blockDim.x)
    for (int d = 0; d < 3; ++d) bad = bad || !icp_finite((double)src[3 * (size_t)p + d]);
  for (int p = tb + threadIdx.x; p < te; p += blockDim.x)
    for (int d = 0; d < 3; ++d) {
      const double v = (double)tgt[3 * (size_t)p + d];
      bad = bad || !icp_finite(v) || (tgt_nrm != nullptr && !icp_finite((double)tgt_nrm[3 * (size_t)p + d]));
      mn[d] = fmin(mn[d], v);
      mx[d] = fmax(mx[d], v);
    }
  if (bad) atomicOr(&sbad, 1);
  for (int d = 0; d < 3; ++d) {
    smn[d][threadIdx.x] = mn[d];
    smx[d][threadIdx.x] = mx[d];
  }
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s)
      for (int d = 0; d < 3; ++d) {
        smn[d][threadIdx.x] = fmin(smn[d][threadIdx.x], smn[d][threadIdx.x + s]);
        smx[d][threadIdx.x] = fmax(smx[d][threadIdx.x], smx[d][threadIdx.x + s]);
      }
    __syncthreads();
  }
  const bool refused = sbad != 0;
  if (refused)  // the pair is finished here: no correspondence, the pose as it came
    for (int p = sb + threadIdx.x; p < se; p += blockDim.x) corr[p] = -1;
  if (threadIdx.x < 12) {
    const double v = pose_init[12 * (size_t)c + threadIdx.x];
    T[12 * (size_t)c + threadIdx.x] = v;
    if (refused) {
      pose64[12 * (size_t)c + threadIdx.x] = v;
      pose[12 * (size_t)c + threadIdx.x] = (float)v;
    }
  }
  if (threadIdx.x != 0) return;
  OvGrid g;
  g.off = 0;
  g.inv_h = 1.0 / h0;
  for (int d = 0; d < 3; ++d) {
    g.mn[d] = 0.0;
    g.dim[d] = 1;
  }
  if (!refused && te > tb) {
    const double bmn[3] = {smn[0][0], smn[1][0], smn[2][0]}, bmx[3] = {smx[0][0], smx[1][0], smx[2][0]};
    (void)ov_fit_grid(bmn, bmx, te - tb, h0, g);  // a grid that does not fit comes back as one cell: slow, not wrong
  }
  info[c] = g;
  prev[2 * c + 0] = prev[2 * c + 1] = 0.0;
  iters[c] = 0;
  done[c] = refused ? 1 : 0;
  status[c] = refused ? -1 : 0;
  if (refused) {
    fitness[c] = rmse[c] = 0.0;
    iterations[c] = count[c] = 0;
    atomicAdd(ndone, 1);
  }
}

// the grids' first cells and blk_cu [nb + 1]: pair c owns the association blocks [blk_cu[c], blk_cu[c + 1])
__global__ void k_icp_offsets(OvGrid* info, const int* __restrict__ src_cu, int nb, int* blk_cu) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  int off = 0, blk = 0;
  for (int c = 0; c < nb; ++c) {
    info[c].off = off;
    off += info[c].dim[0] * info[c].dim[1] * info[c].dim[2];
    blk_cu[c] = blk;
    blk += (src_cu[c + 1] - src_cu[c] + kIcpBlock - 1) / kIcpBlock;
  }
  blk_cu[nb] = blk;
}

__device__ __forceinline__ int icp_cell_of(const OvGrid& g, const float* __restrict__ tgt, int p) {
  int cc[3];
  for (int d = 0; d < 3; ++d)
    cc[d] = min(max(ov_cell((double)tgt[3 * (size_t)p + d], g.mn[d], g.inv_h), 0), g.dim[d] - 1);
  return ov_grid_cell(g, cc[0], cc[1], cc[2]);
}

__global__ __launch_bounds__(256) void k_icp_count(const float* __restrict__ tgt, const int* __restrict__ tgt_cu,
                                                   int nt, int nb, const OvGrid* __restrict__ info, int* count,
                                                   int* cell_of, int* rank) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= nt) return;
  const int c = find_segment(tgt_cu, nb, p);
  const OvGrid g = info[c];
  const int L = icp_cell_of(g, tgt, p);
  cell_of[p] = L;
  rank[p] = atomicAdd(&count[L], 1);  // arrival rank inside the cell
}

__global__ __launch_bounds__(256) void k_icp_scatter(const float* __restrict__ tgt, const int* __restrict__ tgt_cu,
                                                     int nt, int nb, const int* __restrict__ cell_of,
                                                     const int* __restrict__ start, const int* __restrict__ rank,
                                                     OvRec* rec) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= nt) return;
  const int c = find_segment(tgt_cu, nb, p);
  OvRec r;
  r.x = (double)tgt[3 * (size_t)p + 0], r.y = (double)tgt[3 * (size_t)p + 1], r.z = (double)tgt[3 * (size_t)p + 2];
  r.idx = p - tgt_cu[c];
  r.pad = 0;
  rec[start[cell_of[p]] + rank[p]] = r;
}

// One pass of one block: 256 source points of a pair that has not finished.
__global__ __launch_bounds__(256) void k_icp_assoc(const float* __restrict__ src, const int* __restrict__ src_cu,
                                                   const float* __restrict__ tgt, const int* __restrict__ tgt_cu,
                                                   int nb, const int* __restrict__ blk_cu,
                                                   const OvGrid* __restrict__ info, const int* __restrict__ start,
                                                   const OvRec* __restrict__ rec, const double* __restrict__ T,
                                                   const int* __restrict__ done, double r2, int* __restrict__ corr,
                                                   double* __restrict__ part) {
  const int b = blockIdx.x;
  if (b >= blk_cu[nb]) return;
  const int c = find_segment(blk_cu, nb, b);
  if (done[c]) return;
  const int beg = src_cu[c], n = src_cu[c + 1] - beg;
  const int i = (b - blk_cu[c]) * kIcpBlock + threadIdx.x;
  const OvGrid g = info[c];
  double v[kIcpParts];
#pragma unroll
  for (int k = 0; k < kIcpParts; ++k) v[k] = 0.0;
  if (i < n) {
    const double* __restrict__ Tc = T + 12 * (size_t)c;
    const size_t gi = (size_t)(beg + i);
    const double x = (double)src[3 * gi + 0], y = (double)src[3 * gi + 1], z = (double)src[3 * gi + 2];
    double a[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {  // s' = ((R0 x + R1 y) + R2 z) + t, one rounding per operation
      double s = __dadd_rn(__dmul_rn(Tc[4 * k + 0], x), __dmul_rn(Tc[4 * k + 1], y));
      s = __dadd_rn(s, __dmul_rn(Tc[4 * k + 2], z));
      a[k] = __dadd_rn(s, Tc[4 * k + 3]);
    }
    const int cx = ov_cell(a[0], g.mn[0], g.inv_h);
    const int cy = ov_cell(a[1], g.mn[1], g.inv_h);
    const int cz = ov_cell(a[2], g.mn[2], g.inv_h);
    double d2;
    const int j = ov_nearest(rec, ov_runs(g, start, cx, cy, cz), a[0], a[1], a[2], r2, d2);
    corr[gi] = j;
    if (j >= 0) {
      const size_t gj = (size_t)(tgt_cu[c] + j);
      v[0] = 1.0;
      v[16] = d2;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        v[1 + k] = a[k] - g.mn[k];
        v[4 + k] = (double)tgt[3 * gj + k] - g.mn[k];
      }
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int q = 0; q < 3; ++q) v[7 + 3 * r + q] = v[1 + r] * v[4 + q];
    }
  }
  __shared__ double sh[4][kIcpParts];
#pragma unroll
  for (int k = 0; k < kIcpParts; ++k) {
    const double s = wave_sum_d(v[k]);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6][k] = s;
  }
  __syncthreads();
  if (threadIdx.x < kIcpParts)
    part[(size_t)b * kIcpParts + threadIdx.x] =
        ((sh[0][threadIdx.x] + sh[1][threadIdx.x]) + sh[2][threadIdx.x]) + sh[3][threadIdx.x];
}

// What lane 0 of a solve kernel holds of its pair between the end of a pass and the step.
struct IcpPairState {
  double* T;      // [12]
  double* prev;   // fitness and RMSE of the pass before
  int* iters;
  double fit, rms;
};

// The end of a pass, shared by both methods: fitness and RMSE of this evaluation and the stopping rule.  True when the
// pair stops here: its outputs are written and it is frozen.
__device__ __forceinline__ bool icp_pass_end(int c, int n_src, double cnt, double sum_d2, int max_iter,
                                             double rel_fitness, double rel_rmse, IcpPairState& st, int* done,
                                             int* ndone, float* pose, double* pose64, double* fitness, double* rmse,
                                             int* iterations, int* count) {
  st.fit = n_src > 0 ? cnt / (double)n_src : 0.0;
  st.rms = cnt > 0.0 ? sqrt(sum_d2 / cnt) : 0.0;
  const int k = *st.iters;
  const bool converged = k > 0 && fabs(st.fit - st.prev[0]) < rel_fitness && fabs(st.rms - st.prev[1]) < rel_rmse;
  if (k < max_iter && !converged) return false;
  for (int e = 0; e < 12; ++e) {  // the outputs are those of this evaluation
    pose64[12 * (size_t)c + e] = st.T[e];
    pose[12 * (size_t)c + e] = (float)st.T[e];
  }
  fitness[c] = st.fit;
  rmse[c] = st.rms;
  iterations[c] = k;
  count[c] = (int)cnt;
  done[c] = 1;
  atomicAdd(ndone, 1);
  return true;
}

// T <- U o T, and the pass's fitness and RMSE kept for the next stopping test.
__device__ __forceinline__ void icp_step(const double* U, const IcpPairState& st) {
  double* Tc = st.T;
  double N[12];
  for (int r = 0; r < 3; ++r) {
    for (int q = 0; q < 3; ++q)
      N[4 * r + q] = (U[4 * r + 0] * Tc[q] + U[4 * r + 1] * Tc[4 + q]) + U[4 * r + 2] * Tc[8 + q];
    N[4 * r + 3] = ((U[4 * r + 0] * Tc[3] + U[4 * r + 1] * Tc[7]) + U[4 * r + 2] * Tc[11]) + U[4 * r + 3];
  }
  for (int e = 0; e < 12; ++e) Tc[e] = N[e];
  st.prev[0] = st.fit;
  st.prev[1] = st.rms;
  *st.iters += 1;
}

// A x = -g by unpivoted LDL^T in the order of the contract (spr.h); A: the lower triangle is read, the strict lower
// triangle is overwritten by L.  False -- x untouched -- when a pivot is not > 1e-12 max_i A_ii.
__device__ __forceinline__ bool icp_ldlt_solve(double (*A)[6], const double* g, double* x) {
  double m = A[0][0];
#pragma unroll
  for (int i = 1; i < 6; ++i) m = fmax(m, A[i][i]);
  const double floor_d = 1.0e-12 * m;
  double d[6], y[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    double dk = A[k][k];
#pragma unroll
    for (int p = 0; p < k; ++p) dk = dk - (A[k][p] * d[p]) * A[k][p];
    if (!(dk > floor_d)) return false;
    d[k] = dk;
#pragma unroll
    for (int i = k + 1; i < 6; ++i) {
      double s = A[i][k];
#pragma unroll
      for (int p = 0; p < k; ++p) s = s - (A[i][p] * d[p]) * A[k][p];
      A[i][k] = s / dk;
    }
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) {   // L y = -g
    double s = -g[i];
#pragma unroll
    for (int p = 0; p < i; ++p) s = s - A[i][p] * y[p];
    y[i] = s;
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {  // L^T x = D^-1 y
    double s = y[i] / d[i];
#pragma unroll
    for (int p = i + 1; p < 6; ++p) s = s - A[p][i] * x[p];
    x[i] = s;
  }
  return true;
}

// One wave per pair, after every association pass.
__global__ __launch_bounds__(64) void k_icp_solve(const int* __restrict__ src_cu, const int* __restrict__ blk_cu,
                                                  const OvGrid* __restrict__ info, const double* __restrict__ part,
                                                  int max_iter, double rel_fitness, double rel_rmse, double* T,
                                                  double* prev, int* iters, int* done, int* ndone, float* pose,
                                                  double* pose64, double* fitness, double* rmse, int* iterations,
                                                  int* count) {
  const int c = blockIdx.x;
  if (done[c]) return;
  const int b0 = blk_cu[c], b1 = blk_cu[c + 1];
  double S[kIcpParts];
#pragma unroll
  for (int k = 0; k < kIcpParts; ++k) {
    double s = 0.0;
    for (int b = b0 + threadIdx.x; b < b1; b += 64) s += part[(size_t)b * kIcpParts + k];
    S[k] = wave_sum_d(s);
  }
  if (threadIdx.x != 0) return;
  IcpPairState st = {T + 12 * (size_t)c, prev + 2 * c, iters + c, 0.0, 0.0};
  if (icp_pass_end(c, src_cu[c + 1] - src_cu[c], S[0], S[16], max_iter, rel_fitness, rel_rmse, st, done, ndone, pose,
                   pose64, fitness, rmse, iterations, count))
    return;
  const double cnt = S[0];
  double U[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  if (cnt > 0.0) {  // Kabsch on the moments: cov = sum a b^T / n - mean a mean b^T
    const OvGrid g = info[c];
    double ca[3], cb[3], cov[9];
    for (int d = 0; d < 3; ++d) {
      ca[d] = S[1 + d] / cnt;
      cb[d] = S[4 + d] / cnt;
    }
    for (int r = 0; r < 3; ++r)
      for (int q = 0; q < 3; ++q) cov[3 * r + q] = S[7 + 3 * r + q] / cnt - ca[r] * cb[q];
    for (int d = 0; d < 3; ++d) {
      ca[d] += g.mn[d];
      cb[d] += g.mn[d];
    }
    procrustes_pose(cov, ca, cb, U);
  }
  icp_step(U, st);
}

// One pass of one block of the point-to-plane loop: k_icp_assoc's walk, other partials.  kernel 0 / 1 / 2 = L2 /
// Huber / Tukey with parameter kk (spr.h: the weight of a residual).
__global__ __launch_bounds__(256) void k_icp_assoc_plane(
    const float* __restrict__ src, const int* __restrict__ src_cu, const float* __restrict__ tgt,
    const float* __restrict__ tgt_nrm, const int* __restrict__ tgt_cu, int nb, const int* __restrict__ blk_cu,
    const OvGrid* __restrict__ info, const int* __restrict__ start, const OvRec* __restrict__ rec,
    const double* __restrict__ T, const int* __restrict__ done, double r2, int kernel, double kk,
    int* __restrict__ corr, double* __restrict__ part) {
  const int b = blockIdx.x;
  if (b >= blk_cu[nb]) return;
  const int c = find_segment(blk_cu, nb, b);
  if (done[c]) return;
  const int beg = src_cu[c], n = src_cu[c + 1] - beg;
  const int i = (b - blk_cu[c]) * kIcpBlock + threadIdx.x;
  const OvGrid g = info[c];
  double v[kIcpPlaneParts];
#pragma unroll
  for (int k = 0; k < kIcpPlaneParts; ++k) v[k] = 0.0;
  if (i < n) {
    const double* __restrict__ Tc = T + 12 * (size_t)c;
    const size_t gi = (size_t)(beg + i);
    const double x = (double)src[3 * gi + 0], y = (double)src[3 * gi + 1], z = (double)src[3 * gi + 2];
    double a[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {  // s' = ((R0 x + R1 y) + R2 z) + t, one rounding per operation
      double s = __dadd_rn(__dmul_rn(Tc[4 * k + 0], x), __dmul_rn(Tc[4 * k + 1], y));
      s = __dadd_rn(s, __dmul_rn(Tc[4 * k + 2], z));
      a[k] = __dadd_rn(s, Tc[4 * k + 3]);
    }
    const int cx = ov_cell(a[0], g.mn[0], g.inv_h);
    const int cy = ov_cell(a[1], g.mn[1], g.inv_h);
    const int cz = ov_cell(a[2], g.mn[2], g.inv_h);
    double d2;
    const int j = ov_nearest(rec, ov_runs(g, start, cx, cy, cz), a[0], a[1], a[2], r2, d2);
    corr[gi] = j;
    if (j >= 0) {
      const size_t gj = (size_t)(tgt_cu[c] + j);
      double nr[3], e[3], p[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        nr[k] = (double)tgt_nrm[3 * gj + k];
        e[k] = a[k] - (double)tgt[3 * gj + k];
        p[k] = a[k] - g.mn[k];   // g.mn = the target's per-axis minimum: the conditioning shift c of the contract
      }
      const double r = (e[0] * nr[0] + e[1] * nr[1]) + e[2] * nr[2];
      const double J[6] = {p[1] * nr[2] - p[2] * nr[1], p[2] * nr[0] - p[0] * nr[2], p[0] * nr[1] - p[1] * nr[0],
                           nr[0], nr[1], nr[2]};
      const double ar = fabs(r);
      double w = 1.0;
      if (kernel == 1) {
        w = ar <= kk ? 1.0 : kk / ar;
      } else if (kernel == 2) {
        const double q = r / kk, u = 1.0 - q * q;
        w = ar <= kk ? u * u : 0.0;
      }
      v[0] = 1.0;
      v[1] = d2;
      int q = 2;
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        const double wj = w * J[k];
#pragma unroll
        for (int l = k; l < 6; ++l) v[q++] = wj * J[l];
        v[23 + k] = wj * r;
      }
    }
  }
  __shared__ double sh[4][kIcpPlaneParts];
#pragma unroll
  for (int k = 0; k < kIcpPlaneParts; ++k) {
    const double s = wave_sum_d(v[k]);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6][k] = s;
  }
  __syncthreads();
  if (threadIdx.x < kIcpPlaneParts)
    part[(size_t)b * kIcpPlaneParts + threadIdx.x] =
        ((sh[0][threadIdx.x] + sh[1][threadIdx.x]) + sh[2][threadIdx.x]) + sh[3][threadIdx.x];
}

// One wave per pair, after every association pass of the point-to-plane loop.
__global__ __launch_bounds__(64) void k_icp_solve_plane(const int* __restrict__ src_cu, const int* __restrict__ blk_cu,
                                                        const OvGrid* __restrict__ info,
                                                        const double* __restrict__ part, int max_iter,
                                                        double rel_fitness, double rel_rmse, double* T, double* prev,
                                                        int* iters, int* done, int* ndone, float* pose, double* pose64,
                                                        double* fitness, double* rmse, int* iterations, int* count) {
  const int c = blockIdx.x;
  if (done[c]) return;
  const int b0 = blk_cu[c], b1 = blk_cu[c + 1];
  double S[kIcpPlaneParts];
#pragma unroll
  for (int k = 0; k < kIcpPlaneParts; ++k) {
    double s = 0.0;
    for (int b = b0 + threadIdx.x; b < b1; b += 64) s += part[(size_t)b * kIcpPlaneParts + k];
    S[k] = wave_sum_d(s);
  }
  if (threadIdx.x != 0) return;
  IcpPairState st = {T + 12 * (size_t)c, prev + 2 * c, iters + c, 0.0, 0.0};
  if (icp_pass_end(c, src_cu[c + 1] - src_cu[c], S[0], S[1], max_iter, rel_fitness, rel_rmse, st, done, ndone, pose,
                   pose64, fitness, rmse, iterations, count))
    return;
  double U[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  double A[6][6], x[6];
  {
    int q = 2;
#pragma unroll
    for (int k = 0; k < 6; ++k)
#pragma unroll
      for (int l = k; l < 6; ++l) A[l][k] = S[q++];   // the lower triangle is what the factorisation reads
  }
  if (S[0] > 0.0 && icp_ldlt_solve(A, S + 23, x)) {
    const double* cc = info[c].mn;
    const double sx = sin(x[0]), cx = cos(x[0]), sy = sin(x[1]), cy = cos(x[1]), sz = sin(x[2]), cz = cos(x[2]);
    U[0] = cz * cy, U[1] = (cz * sy) * sx - sz * cx, U[2] = (cz * sy) * cx + sz * sx;
    U[4] = sz * cy, U[5] = (sz * sy) * sx + cz * cx, U[6] = (sz * sy) * cx - cz * sx;
    U[8] = -sy, U[9] = cy * sx, U[10] = cy * cx;
    U[3] = x[3] - (x[1] * cc[2] - x[2] * cc[1]);   // t = v - omega x c: the step about the world origin
    U[7] = x[4] - (x[2] * cc[0] - x[0] * cc[2]);
    U[11] = x[5] - (x[0] * cc[1] - x[1] * cc[0]);
  }
  icp_step(U, st);
}

struct IcpWs {
  OvGrid* info;
  int *blk_cu, *done, *iters, *ndone;
  double *T, *prev;
  int *count, *start, *cell_of, *rank;
  OvRec* rec;
  double* part;
  void* temp;
  size_t cells, temp_bytes;
};
IcpWs icp_layout(Workspace& w, int ns, int nt, int nb, int parts) {
  IcpWs l;
  const size_t B = nb > 0 ? nb : 1, M = nt > 0 ? nt : 1;   // the query measures nb = 0 as one pair
  l.cells = (size_t)kOvCellsPerPoint * (size_t)nt + (size_t)kOvCellsBase * B;
  l.info = w.take<OvGrid>(B);
  l.blk_cu = w.take<int>(B + 1);
  l.done = w.take<int>(B);
  l.iters = w.take<int>(B);
  l.ndone = w.take<int>(64);
  l.T = w.take<double>(12 * B);
  l.prev = w.take<double>(2 * B);
  l.count = w.take<int>(l.cells + 1);
  l.start = w.take<int>(l.cells + 1);
  l.cell_of = w.take<int>(M);
  l.rank = w.take<int>(M);
  l.rec = w.take<OvRec>(M);
  l.part = w.take<double>((size_t)parts * ((size_t)cdiv(ns, kIcpBlock) + B));
  l.temp_bytes = ov_scan_temp_bytes(l.cells + 1);
  l.temp = w.take<char>(l.temp_bytes);
  return l;
}

// Both entry points: `what` names the caller in messages; tgt_nrm == nullptr with plane == false is point-to-point.
struct IcpCall {
  const char* what;
  bool plane;
  const float* tgt_nrm;
  int kernel;
  double kernel_k;
};

int icp_run(const IcpCall& m, const float* src_xyz, const int* src_cu, int ns, const float* tgt_xyz, const int* tgt_cu,
            int nt, const double* pose_init, int nb, double max_dist, int max_iter, double rel_fitness, double rel_rmse,
            float* pose, double* pose64, double* fitness, double* inlier_rmse, int* iterations, int* count, int* corr,
            int* status, void* ws, size_t ws_bytes, hipStream_t stream) {
  SPR_REQUIRE(nb >= 0 && ns >= 0 && nt >= 0, "%s: negative size (nb=%d ns=%d nt=%d)", m.what, nb, ns, nt);
  SPR_REQUIRE(max_dist > 0.0 && max_dist < 1.0e150, "%s: max_dist must be > 0 (and finite), got %g", m.what, max_dist);
  SPR_REQUIRE(max_iter >= 0, "%s: max_iter must be >= 0, got %d", m.what, max_iter);
  SPR_REQUIRE(rel_fitness == rel_fitness && rel_rmse == rel_rmse, "%s: rel_fitness / rel_rmse is NaN", m.what);
  if (m.plane) {
    SPR_REQUIRE(m.kernel >= 0 && m.kernel <= 2, "%s: kernel must be 0 (L2), 1 (Huber) or 2 (Tukey), got %d", m.what,
                m.kernel);
    SPR_REQUIRE(m.kernel == 0 || (m.kernel_k > 0.0 && m.kernel_k < 1.0e150),
                "%s: kernel_k must be > 0 (and finite) with a robust kernel, got %g", m.what, m.kernel_k);
  }
  SPR_REQUIRE(nb < 32768, "%s: at most 32767 pairs per call", m.what);
  SPR_REQUIRE((size_t)ns + (size_t)nt <= ((size_t)1 << 26), "%s: at most 2^26 points per call", m.what);
  SPR_REQUIRE(nb > 0 || (ns == 0 && nt == 0), "%s: points without pairs (nb=0 ns=%d nt=%d)", m.what, ns, nt);
  if (nb == 0) return 0;
  SPR_REQUIRE(src_cu && tgt_cu && pose_init, "%s: src_cu, tgt_cu and pose_init must not be null", m.what);
  SPR_REQUIRE(pose && pose64 && fitness && inlier_rmse && iterations && count && status, "%s: null per-pair output",
              m.what);
  SPR_REQUIRE(ns == 0 || (src_xyz && corr), "%s: null source pointer with ns=%d", m.what, ns);
  SPR_REQUIRE(nt == 0 || (tgt_xyz && (!m.plane || m.tgt_nrm)), "%s: null target pointer with nt=%d", m.what, nt);
  const int parts = m.plane ? kIcpPlaneParts : kIcpParts;
  Workspace w(ws, ws_bytes);
  const IcpWs l = icp_layout(w, ns, nt, nb, parts);
  SPR_REQUIRE(ws != nullptr && w.ok(), "%s: workspace too small", m.what);

  const double h0 = max_dist * (1.0 + 1.0 / 256.0);
  const double r2 = max_dist * max_dist;
  const int TB = 256;
  SPR_HIP_CHECK(hipMemsetAsync(l.ndone, 0, 64 * sizeof(int), stream));
  SPR_HIP_CHECK(hipMemsetAsync(l.count, 0, (l.cells + 1) * sizeof(int), stream));
  hipLaunchKernelGGL(k_icp_setup, dim3(nb), dim3(256), 0, stream, src_xyz, src_cu, tgt_xyz, tgt_cu,
                     m.plane ? m.tgt_nrm : nullptr, pose_init, h0, l.info, l.T, l.prev, l.iters, l.done, l.ndone, pose,
                     pose64, fitness, inlier_rmse, iterations, count, corr, status);
  hipLaunchKernelGGL(k_icp_offsets, dim3(1), dim3(64), 0, stream, l.info, src_cu, nb, l.blk_cu);
  if (nt > 0)
    hipLaunchKernelGGL(k_icp_count, dim3(cdiv(nt, TB)), dim3(TB), 0, stream, tgt_xyz, tgt_cu, nt, nb, l.info, l.count,
                       l.cell_of, l.rank);
  SPR_LAUNCH_CHECK();
  size_t tb = l.temp_bytes;
  SPR_HIP_CHECK(rocprim::exclusive_scan(l.temp, tb, l.count, l.start, 0, l.cells + 1, rocprim::plus<int>(), stream));
  if (nt > 0)
    hipLaunchKernelGGL(k_icp_scatter, dim3(cdiv(nt, TB)), dim3(TB), 0, stream, tgt_xyz, tgt_cu, nt, nb, l.cell_of,
                       l.start, l.rank, l.rec);
  SPR_LAUNCH_CHECK();

  const int nblk = cdiv(ns, kIcpBlock) + nb;
  for (int pass = 0; pass <= max_iter;) {
    const int stop = pass + kIcpChunk < max_iter + 1 ? pass + kIcpChunk : max_iter + 1;
    for (; pass < stop; ++pass) {
      if (m.plane) {
        hipLaunchKernelGGL(k_icp_assoc_plane, dim3(nblk), dim3(kIcpBlock), 0, stream, src_xyz, src_cu, tgt_xyz,
                           m.tgt_nrm, tgt_cu, nb, l.blk_cu, l.info, l.start, l.rec, l.T, l.done, r2, m.kernel,
                           m.kernel_k, corr, l.part);
        hipLaunchKernelGGL(k_icp_solve_plane, dim3(nb), dim3(64), 0, stream, src_cu, l.blk_cu, l.info, l.part,
                           max_iter, rel_fitness, rel_rmse, l.T, l.prev, l.iters, l.done, l.ndone, pose, pose64,
                           fitness, inlier_rmse, iterations, count);
      } else {
        hipLaunchKernelGGL(k_icp_assoc, dim3(nblk), dim3(kIcpBlock), 0, stream, src_xyz, src_cu, tgt_xyz, tgt_cu, nb,
                           l.blk_cu, l.info, l.start, l.rec, l.T, l.done, r2, corr, l.part);
        hipLaunchKernelGGL(k_icp_solve, dim3(nb), dim3(64), 0, stream, src_cu, l.blk_cu, l.info, l.part, max_iter,
                           rel_fitness, rel_rmse, l.T, l.prev, l.iters, l.done, l.ndone, pose, pose64, fitness,
                           inlier_rmse, iterations, count);
      }
    }
    SPR_LAUNCH_CHECK();
    if (pass > max_iter) break;   // the last pass finishes every pair: nothing to ask
    int finished = 0;
    SPR_HIP_CHECK(hipMemcpyAsync(&finished, l.ndone, sizeof(int), hipMemcpyDeviceToHost, stream));
    SPR_HIP_CHECK(hipStreamSynchronize(stream));
    if (finished >= nb) break;
  }
  return 0;
}

}  // namespace
}  // namespace spr

using namespace spr;

extern "C" size_t spr_icp_pairs_workspace_size(int ns, int nt, int nb) {
  if (ns < 0 || nt < 0 || nb < 0) return 0;
  return measure(icp_layout, ns, nt, nb, kIcpParts);
}

extern "C" int spr_icp_pairs(const float* src_xyz, const int* src_cu, int ns, const float* tgt_xyz, const int* tgt_cu,
                             int nt, const double* pose_init, int nb, double max_dist, int max_iter,
                             double rel_fitness, double rel_rmse, float* pose, double* pose64, double* fitness,
                             double* inlier_rmse, int* iterations, int* count, int* corr, int* status, void* ws,
                             size_t ws_bytes, void* stream) {
  const IcpCall m = {"icp_pairs", false, nullptr, 0, 0.0};
  return icp_run(m, src_xyz, src_cu, ns, tgt_xyz, tgt_cu, nt, pose_init, nb, max_dist, max_iter, rel_fitness, rel_rmse,
                 pose, pose64, fitness, inlier_rmse, iterations, count, corr, status, ws, ws_bytes, (hipStream_t)stream);
}

extern "C" size_t spr_icp_plane_pairs_workspace_size(int ns, int nt, int nb) {
  if (ns < 0 || nt < 0 || nb < 0) return 0;
  return measure(icp_layout, ns, nt, nb, kIcpPlaneParts);
}

extern "C" int spr_icp_plane_pairs(const float* src_xyz, const int* src_cu, int ns, const float* tgt_xyz,
                                   const float* tgt_normals, const int* tgt_cu, int nt, const double* pose_init, int nb,
                                   double max_dist, int max_iter, double rel_fitness, double rel_rmse, int kernel,
                                   double kernel_k, float* pose, double* pose64, double* fitness, double* inlier_rmse,
                                   int* iterations, int* count, int* corr, int* status, void* ws, size_t ws_bytes,
                                   void* stream) {
  const IcpCall m = {"icp_plane_pairs", true, tgt_normals, kernel, kernel_k};
  return icp_run(m, src_xyz, src_cu, ns, tgt_xyz, tgt_cu, nt, pose_init, nb, max_dist, max_iter, rel_fitness, rel_rmse,
                 pose, pose64, fitness, inlier_rmse, iterations, count, corr, status, ws, ws_bytes, (hipStream_t)stream);
}
