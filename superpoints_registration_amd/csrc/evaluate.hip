// Registration metrics for all pairs of a batch in one call, on gfx950: the RPMNet / DCP table the reference prints on
// ModelNet (benchmark/benchmark_modelnet.py: compute_metrics), se3_compare's translation error and the inlier ratio of
// a set of correspondences (models/generic_reg_model.py: compute_IR).
//
// Behaviour contract: include/spr.h, "Registration metrics for all pairs" -- a float64 definition per pair, one
// rounding per operation, no FMA (the file is built with -ffp-contract=off like every other one).  The reference
// materialises [B, n, m, 3] differences in torch and is only right at batch size 1; here
//   k_eval_setup      one workgroup per pair: the non-finite test of every input of the pair; the strict-threshold
//                     inlier count (integers: order free); in lane 0 the pose algebra (Ginv, C = Ginv o P,
//                     D = P o Ginv), the Euler / translation / isotropic columns and the pair's status; P and D go to
//                     the workspace for the transform
//   k_eval_offsets    blk_cu [2 nb + 1]: segment 2 c + dir owns the search blocks of pair c, direction dir
//   k_eval_transform  every source point by P and every raw point by D, ONCE, into the workspace (float64 rows)
//   k_eval_nn         exact brute-force nearest neighbour in float64 for the queries of all pairs and both directions:
//                     one wave per block of kEvalQ = 128 queries, kEvalQPL = 2 queries per lane in registers; the
//                     targets of the pair go through LDS in tiles of kEvalT = 256 points as SoA doubles, and every
//                     target is ONE broadcast read per coordinate for the lane's queries.  Strict "<" over
//                     ascending j keeps the lowest index of a tie.  Per block one float64 partial: the sum of its d2
//   k_eval_finish     one wave per pair: the partials of each direction added lane-strided, then by wave shuffles ->
//                     chamfer_src, chamfer_ref, chamfer_dist
// Cost: O(n m) per pair and direction -- 8 float64 operations, one compare and three selects per (query, target).  That
// is the right trade for object-sized clouds (ModelNet: 717 x 2048); a grid-accelerated search for scan-sized clouds
// is out of scope.
//
// Order of the sums: block b of a segment holds its queries [128 b, 128 b + 128); lane l holds queries
// 128 b + 64 k + l, k = 0, 1, added as q0 + q1, then wave shuffles (xor 32 .. 1); k_eval_finish adds
// the blocks' partials lane-strided (lane l takes blocks l, l + 64, ..), then wave shuffles.  All of it is a function of
// the pair alone -- no floating-point atomics -- so every output of a pair has the same bits whatever batch it is
// called in, and run to run.
#include "spr_common.h"

namespace spr {
namespace {

constexpr int kEvalT = SPR_EVAL_TILE;      // targets per LDS tile
constexpr int kEvalQ = SPR_EVAL_QUERIES;   // queries per workgroup (one wave)
constexpr int kEvalQPL = kEvalQ / 64;      // queries per lane
static_assert(kEvalQPL * 64 == kEvalQ && kEvalT % 64 == 0, "tile constants");

// column indices of metrics [nb, SPR_EVAL_COLS] (spr.h)
enum { R_MSE, R_MAE, T_MSE, T_MAE, ERR_R, ERR_T, TRANS_ERR, CH_SRC, CH_REF, CH_DIST, IN_COUNT, IN_RATIO };
static_assert(IN_RATIO + 1 == SPR_EVAL_COLS, "metric columns");

__device__ __forceinline__ bool eval_finite(double v) { return fabs(v) < 1.0e300; }

__device__ __forceinline__ double eval_dot3(double a0, double b0, double a1, double b1, double a2, double b2) {
  return __dadd_rn(__dadd_rn(__dmul_rn(a0, b0), __dmul_rn(a1, b1)), __dmul_rn(a2, b2));
}
// row k of T applied to (x, y, z): ((R0 x + R1 y) + R2 z) + t
__device__ __forceinline__ double eval_row(const double* __restrict__ T, int k, double x, double y, double z) {
  return __dadd_rn(eval_dot3(T[4 * k + 0], x, T[4 * k + 1], y, T[4 * k + 2], z), T[4 * k + 3]);
}
__device__ __forceinline__ double eval_d2(double ax, double ay, double az, double bx, double by, double bz) {
  const double dx = __dsub_rn(ax, bx), dy = __dsub_rn(ay, by), dz = __dsub_rn(az, bz);
  return __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
}
// A o B for [3,4] poses (apply B first)
__device__ __forceinline__ void eval_compose(const double* A, const double* B, double* O) {
  for (int r = 0; r < 3; ++r) {
    for (int q = 0; q < 3; ++q) O[4 * r + q] = eval_dot3(A[4 * r], B[q], A[4 * r + 1], B[4 + q], A[4 * r + 2], B[8 + q]);
    O[4 * r + 3] = __dadd_rn(eval_dot3(A[4 * r], B[3], A[4 * r + 1], B[7], A[4 * r + 2], B[11]), A[4 * r + 3]);
  }
}
__device__ __forceinline__ double eval_clamp1(double v) { return fmin(fmax(v, -1.0), 1.0); }
__device__ __forceinline__ double eval_deg(double rad) { return rad * 180.0 / 3.141592653589793; }
// scipy's as_euler('xyz', degrees=True) away from gimbal lock
__device__ __forceinline__ void eval_euler(const double* T, double* e) {
  e[0] = eval_deg(atan2(T[9], T[10]));
  e[1] = eval_deg(-asin(eval_clamp1(T[8])));
  e[2] = eval_deg(atan2(T[4], T[0]));
}
__device__ __forceinline__ double eval_norm3(double x, double y, double z) {
  return sqrt(__dadd_rn(__dadd_rn(__dmul_rn(x, x), __dmul_rn(y, y)), __dmul_rn(z, z)));
}

__device__ __forceinline__ bool eval_cloud_bad(const float* __restrict__ xyz, int beg, int end) {
  bool bad = false;
  for (int p = beg + (int)threadIdx.x; p < end; p += (int)blockDim.x)
    for (int d = 0; d < 3; ++d) bad = bad || !eval_finite((double)xyz[3 * (size_t)p + d]);
  return bad;
}

// One workgroup per pair.  raw / corr_* may be null (with their cu arrays): that part is not asked for.
__global__ __launch_bounds__(256) void k_eval_setup(
    const float* __restrict__ src, const int* __restrict__ src_cu, const float* __restrict__ ref,
    const int* __restrict__ ref_cu, const float* __restrict__ raw, const int* __restrict__ raw_cu,
    const float* __restrict__ corr_src, const float* __restrict__ corr_tgt, const int* __restrict__ corr_cu,
    const double* __restrict__ pose_gt, const double* __restrict__ pose_pred, double r2, double* __restrict__ TP,
    double* __restrict__ TD, double* __restrict__ metrics, int* __restrict__ status) {
  const int c = blockIdx.x;
  __shared__ int sbad, scount;
  if (threadIdx.x == 0) sbad = scount = 0;
  __syncthreads();
  const double* __restrict__ G = pose_gt + 12 * (size_t)c;
  const double* __restrict__ P = pose_pred + 12 * (size_t)c;
  bool bad = false;
  if (threadIdx.x < 12) bad = !eval_finite(G[threadIdx.x]) || !eval_finite(P[threadIdx.x]);
  bad = bad || eval_cloud_bad(src, src_cu[c], src_cu[c + 1]) || eval_cloud_bad(ref, ref_cu[c], ref_cu[c + 1]);
  if (raw_cu != nullptr) bad = bad || eval_cloud_bad(raw, raw_cu[c], raw_cu[c + 1]);
  int cnt = 0, ncorr = 0;
  if (corr_cu != nullptr) {
    const int kb = corr_cu[c], ke = corr_cu[c + 1];
    ncorr = ke - kb;
    bad = bad || eval_cloud_bad(corr_src, kb, ke) || eval_cloud_bad(corr_tgt, kb, ke);
    for (int k = kb + (int)threadIdx.x; k < ke; k += (int)blockDim.x) {
      const double x = (double)corr_src[3 * (size_t)k], y = (double)corr_src[3 * (size_t)k + 1],
                   z = (double)corr_src[3 * (size_t)k + 2];
      const double d2 = eval_d2(eval_row(G, 0, x, y, z), eval_row(G, 1, x, y, z), eval_row(G, 2, x, y, z),
                                (double)corr_tgt[3 * (size_t)k], (double)corr_tgt[3 * (size_t)k + 1],
                                (double)corr_tgt[3 * (size_t)k + 2]);
      cnt += d2 < r2 ? 1 : 0;
    }
  }
  if (bad) atomicOr(&sbad, 1);
  if (cnt) atomicAdd(&scount, cnt);   // integers: the order of arrival does not matter
  __syncthreads();
  if (threadIdx.x != 0) return;
  double* __restrict__ m = metrics + (size_t)SPR_EVAL_COLS * c;
  for (int k = 0; k < SPR_EVAL_COLS; ++k) m[k] = 0.0;
  double* __restrict__ tp = TP + 12 * (size_t)c;
  double* __restrict__ td = TD + 12 * (size_t)c;
  if (sbad) {
    status[c] = -1;
    for (int e = 0; e < 12; ++e) tp[e] = td[e] = 0.0;   // never applied: the pair's blocks leave on its status
    return;
  }
  const bool no_raw = raw_cu != nullptr && raw_cu[c + 1] == raw_cu[c] &&
                      (src_cu[c + 1] > src_cu[c] || ref_cu[c + 1] > ref_cu[c]);
  status[c] = no_raw ? -2 : 0;
  double g[12], p[12], Gi[12], C[12], D[12];
  for (int e = 0; e < 12; ++e) {
    g[e] = G[e];
    p[e] = P[e];
  }
  for (int r = 0; r < 3; ++r) {   // Ginv = [Rg^T | -(Rg^T tg)]
    for (int q = 0; q < 3; ++q) Gi[4 * r + q] = g[4 * q + r];
    Gi[4 * r + 3] = -eval_dot3(g[r], g[3], g[4 + r], g[7], g[8 + r], g[11]);
  }
  eval_compose(Gi, p, C);
  eval_compose(p, Gi, D);
  for (int e = 0; e < 12; ++e) {
    tp[e] = p[e];
    td[e] = D[e];
  }
  double eg[3], ep[3], dr[3], dt[3];
  eval_euler(g, eg);
  eval_euler(p, ep);
  for (int k = 0; k < 3; ++k) {
    dr[k] = eg[k] - ep[k];
    dt[k] = g[4 * k + 3] - p[4 * k + 3];
  }
  m[R_MSE] = ((dr[0] * dr[0] + dr[1] * dr[1]) + dr[2] * dr[2]) / 3.0;
  m[R_MAE] = ((fabs(dr[0]) + fabs(dr[1])) + fabs(dr[2])) / 3.0;
  m[T_MSE] = ((dt[0] * dt[0] + dt[1] * dt[1]) + dt[2] * dt[2]) / 3.0;
  m[T_MAE] = ((fabs(dt[0]) + fabs(dt[1])) + fabs(dt[2])) / 3.0;
  m[ERR_R] = eval_deg(acos(eval_clamp1(0.5 * (((C[0] + C[5]) + C[10]) - 1.0))));
  m[ERR_T] = eval_norm3(C[3], C[7], C[11]);
  m[TRANS_ERR] = eval_norm3(D[3], D[7], D[11]);
  m[IN_COUNT] = (double)scount;
  m[IN_RATIO] = ncorr > 0 ? (double)scount / (double)ncorr : 0.0;
}

// blk_cu [2 nb + 1]: segment 2 c owns the blocks of pair c's source queries, 2 c + 1 those of its reference queries
__global__ void k_eval_offsets(const int* __restrict__ src_cu, const int* __restrict__ ref_cu, int nb, int* blk_cu) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  int blk = 0;
  for (int c = 0; c < nb; ++c) {
    blk_cu[2 * c] = blk;
    blk += (src_cu[c + 1] - src_cu[c] + kEvalQ - 1) / kEvalQ;
    blk_cu[2 * c + 1] = blk;
    blk += (ref_cu[c + 1] - ref_cu[c] + kEvalQ - 1) / kEvalQ;
  }
  blk_cu[2 * nb] = blk;
}

// rows [0, ns): source point by P -> A; rows [ns, ns + nr): raw point by D -> Cr
__global__ __launch_bounds__(256) void k_eval_transform(const float* __restrict__ src, const int* __restrict__ src_cu,
                                                        int ns, const float* __restrict__ raw,
                                                        const int* __restrict__ raw_cu, int nr, int nb,
                                                        const double* __restrict__ TP, const double* __restrict__ TD,
                                                        double* __restrict__ A, double* __restrict__ Cr) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ns + nr) return;
  const bool is_raw = i >= ns;
  const int p = is_raw ? i - ns : i;
  const float* __restrict__ xyz = is_raw ? raw : src;
  const int c = find_segment(is_raw ? raw_cu : src_cu, nb, p);
  const double* __restrict__ T = (is_raw ? TD : TP) + 12 * (size_t)c;
  double* __restrict__ out = (is_raw ? Cr : A) + 3 * (size_t)p;
  const double x = (double)xyz[3 * (size_t)p], y = (double)xyz[3 * (size_t)p + 1], z = (double)xyz[3 * (size_t)p + 2];
  out[0] = eval_row(T, 0, x, y, z);
  out[1] = eval_row(T, 1, x, y, z);
  out[2] = eval_row(T, 2, x, y, z);
}

// One wave per block of kEvalQ queries of one pair and one direction.
//   dir 0: queries A (the moved source, float64), targets raw (float32, converted exactly)
//   dir 1: queries ref (float32),                 targets Cr (the moved raw shape, float64)
__global__ __launch_bounds__(64) void k_eval_nn(const int* __restrict__ src_cu, const float* __restrict__ ref,
                                                const int* __restrict__ ref_cu, const float* __restrict__ raw,
                                                const int* __restrict__ raw_cu, int nb,
                                                const int* __restrict__ blk_cu, const double* __restrict__ A,
                                                const double* __restrict__ Cr, const int* __restrict__ status,
                                                double* __restrict__ d2_src, int* __restrict__ nn_src,
                                                double* __restrict__ d2_ref, int* __restrict__ nn_ref,
                                                double* __restrict__ part) {
  const int b = blockIdx.x;
  if (b >= blk_cu[2 * nb]) return;
  const int s = find_segment(blk_cu, 2 * nb, b);
  const int c = s >> 1, dir = s & 1;
  const int* __restrict__ qcu = dir ? ref_cu : src_cu;
  const int qbeg = qcu[c], nq = qcu[c + 1] - qbeg;
  const int q0 = (b - blk_cu[s]) * kEvalQ;
  const int rbeg = raw_cu[c], m = raw_cu[c + 1] - rbeg;
  double* __restrict__ d2_out = dir ? d2_ref : d2_src;
  int* __restrict__ nn_out = dir ? nn_ref : nn_src;
  const int lane = threadIdx.x;
  const bool live = status[c] == 0;   // uniform over the block; a live pair with queries has m > 0

  double qx[kEvalQPL], qy[kEvalQPL], qz[kEvalQPL], best[kEvalQPL];
  int idx[kEvalQPL];
#pragma unroll
  for (int k = 0; k < kEvalQPL; ++k) {
    const int i = q0 + 64 * k + lane;
    qx[k] = qy[k] = qz[k] = 0.0;
    best[k] = __builtin_huge_val();
    idx[k] = 0;
    if (live && i < nq) {
      const size_t gi = (size_t)(qbeg + i);
      if (dir) {
        qx[k] = (double)ref[3 * gi], qy[k] = (double)ref[3 * gi + 1], qz[k] = (double)ref[3 * gi + 2];
      } else {
        qx[k] = A[3 * gi], qy[k] = A[3 * gi + 1], qz[k] = A[3 * gi + 2];
      }
    }
  }
  __shared__ double sx[kEvalT], sy[kEvalT], sz[kEvalT];
  if (live) {
    for (int t0 = 0; t0 < m; t0 += kEvalT) {
      const int tn = min(kEvalT, m - t0);
      __syncthreads();   // the tile before has been read by every lane
      for (int j = lane; j < tn; j += 64) {
        const size_t gj = (size_t)(rbeg + t0 + j);
        if (dir) {
          sx[j] = Cr[3 * gj], sy[j] = Cr[3 * gj + 1], sz[j] = Cr[3 * gj + 2];
        } else {
          sx[j] = (double)raw[3 * gj], sy[j] = (double)raw[3 * gj + 1], sz[j] = (double)raw[3 * gj + 2];
        }
      }
      __syncthreads();
#pragma unroll 4
      for (int j = 0; j < tn; ++j) {
        const double tx = sx[j], ty = sy[j], tz = sz[j];   // one broadcast read each for the lane's queries
#pragma unroll
        for (int k = 0; k < kEvalQPL; ++k) {
          const double d = eval_d2(qx[k], qy[k], qz[k], tx, ty, tz);
          const bool lt = d < best[k];   // strict, j ascending: the lowest index of a tie stays
          best[k] = lt ? d : best[k];
          idx[k] = lt ? t0 + j : idx[k];
        }
      }
    }
  }
  double sum = 0.0;
#pragma unroll
  for (int k = 0; k < kEvalQPL; ++k) {
    const int i = q0 + 64 * k + lane;
    const bool mine = i < nq;
    const double v = live && mine ? best[k] : 0.0;
    if (mine) {
      const size_t gi = (size_t)(qbeg + i);
      if (d2_out != nullptr) d2_out[gi] = v;
      if (nn_out != nullptr) nn_out[gi] = live ? idx[k] : -1;
    }
    sum = k == 0 ? v : sum + v;
  }
  sum = wave_sum_d(sum);
  if (lane == 0) part[b] = sum;
}

// Queries of a pair that has no search (raw not given is handled on the host; status != 0 inside k_eval_nn).
// One wave per pair: the Chamfer columns.
__global__ __launch_bounds__(64) void k_eval_finish(const int* __restrict__ src_cu, const int* __restrict__ ref_cu,
                                                    const int* __restrict__ blk_cu, const double* __restrict__ part,
                                                    const int* __restrict__ status, double* __restrict__ metrics) {
  const int c = blockIdx.x;
  if (status[c] != 0) return;   // uniform; the columns are already 0
  double S[2];
  for (int dir = 0; dir < 2; ++dir) {
    double s = 0.0;
    for (int b = blk_cu[2 * c + dir] + (int)threadIdx.x; b < blk_cu[2 * c + dir + 1]; b += 64) s += part[b];
    S[dir] = wave_sum_d(s);
  }
  if (threadIdx.x != 0) return;
  const int n_src = src_cu[c + 1] - src_cu[c], n_ref = ref_cu[c + 1] - ref_cu[c];
  double* __restrict__ m = metrics + (size_t)SPR_EVAL_COLS * c;
  m[CH_SRC] = n_src > 0 ? S[0] / (double)n_src : 0.0;
  m[CH_REF] = n_ref > 0 ? S[1] / (double)n_ref : 0.0;
  m[CH_DIST] = m[CH_SRC] + m[CH_REF];
}

struct EvalWs {
  double *TP, *TD, *A, *Cr, *part;
  int* blk_cu;
};
EvalWs eval_layout(Workspace& w, int ns, int nt, int nr, int nc, int nb) {
  (void)nc;   // correspondences are consumed where they are read
  EvalWs l;
  const size_t B = nb > 0 ? nb : 1;   // the query measures nb = 0 as one pair
  l.TP = w.take<double>(12 * B);
  l.TD = w.take<double>(12 * B);
  l.blk_cu = w.take<int>(2 * B + 1);
  l.A = w.take<double>(3 * (size_t)(ns > 0 ? ns : 1));
  l.Cr = w.take<double>(3 * (size_t)(nr > 0 ? nr : 1));
  l.part = w.take<double>((size_t)cdiv(ns, kEvalQ) + (size_t)cdiv(nt, kEvalQ) + 2 * B);
  return l;
}

}  // namespace
}  // namespace spr

using namespace spr;

extern "C" size_t spr_eval_pairs_workspace_size(int ns, int nt, int nr, int nc, int nb) {
  if (ns < 0 || nt < 0 || nr < 0 || nc < 0 || nb < 0) return 0;
  return measure(eval_layout, ns, nt, nr, nc, nb);
}

extern "C" int spr_eval_pairs(const float* src_xyz, const int* src_cu, int ns, const float* ref_xyz, const int* ref_cu,
                              int nt, const float* raw_xyz, const int* raw_cu, int nr, const float* corr_src,
                              const float* corr_tgt, const int* corr_cu, int nc, const double* pose_gt,
                              const double* pose_pred, int nb, double acceptance_radius, double* metrics,
                              double* d2_src, int* nn_src, double* d2_ref, int* nn_ref, int* status, void* ws,
                              size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPR_REQUIRE(nb >= 0 && ns >= 0 && nt >= 0 && nr >= 0 && nc >= 0,
              "eval_pairs: negative size (nb=%d ns=%d nt=%d nr=%d nc=%d)", nb, ns, nt, nr, nc);
  SPR_REQUIRE(nb < 32768, "eval_pairs: at most 32767 pairs per call");
  SPR_REQUIRE((size_t)ns + (size_t)nt + (size_t)nr + (size_t)nc <= ((size_t)1 << 26),
              "eval_pairs: at most 2^26 points per call");
  SPR_REQUIRE(nb > 0 || (ns == 0 && nt == 0 && nr == 0 && nc == 0),
              "eval_pairs: points without pairs (nb=0 ns=%d nt=%d nr=%d nc=%d)", ns, nt, nr, nc);
  const bool chamfer = raw_cu != nullptr, inliers = corr_cu != nullptr;
  SPR_REQUIRE(chamfer || nr == 0, "eval_pairs: nr=%d without raw_cu", nr);
  SPR_REQUIRE(inliers || nc == 0, "eval_pairs: nc=%d without corr_cu", nc);
  SPR_REQUIRE(!inliers || (acceptance_radius > 0.0 && acceptance_radius < 1.0e150),
              "eval_pairs: acceptance_radius must be > 0 (and finite) with correspondences, got %g", acceptance_radius);
  if (nb == 0) return 0;
  SPR_REQUIRE(src_cu && ref_cu && pose_gt && pose_pred, "eval_pairs: src_cu, ref_cu and the poses must not be null");
  SPR_REQUIRE(metrics && status, "eval_pairs: null per-pair output");
  SPR_REQUIRE(ns == 0 || src_xyz, "eval_pairs: null source pointer with ns=%d", ns);
  SPR_REQUIRE(nt == 0 || ref_xyz, "eval_pairs: null reference pointer with nt=%d", nt);
  SPR_REQUIRE(nr == 0 || raw_xyz, "eval_pairs: null raw pointer with nr=%d", nr);
  SPR_REQUIRE(nc == 0 || (corr_src && corr_tgt), "eval_pairs: null correspondence pointer with nc=%d", nc);
  Workspace w(ws, ws_bytes);
  const EvalWs l = eval_layout(w, ns, nt, nr, nc, nb);
  SPR_REQUIRE(ws != nullptr && w.ok(), "eval_pairs: workspace too small");

  const double r2 = inliers ? acceptance_radius * acceptance_radius : 0.0;
  hipLaunchKernelGGL(k_eval_setup, dim3(nb), dim3(256), 0, stream, src_xyz, src_cu, ref_xyz, ref_cu, raw_xyz, raw_cu,
                     corr_src, corr_tgt, corr_cu, pose_gt, pose_pred, r2, l.TP, l.TD, metrics, status);
  if (chamfer) {
    const int nblk = cdiv(ns, kEvalQ) + cdiv(nt, kEvalQ) + 2 * nb;   // >= blk_cu[2 nb]; the rest leaves at once
    hipLaunchKernelGGL(k_eval_offsets, dim3(1), dim3(64), 0, stream, src_cu, ref_cu, nb, l.blk_cu);
    if (ns + nr > 0)
      hipLaunchKernelGGL(k_eval_transform, dim3(cdiv((long)ns + nr, 256)), dim3(256), 0, stream, src_xyz, src_cu, ns,
                         raw_xyz, raw_cu, nr, nb, l.TP, l.TD, l.A, l.Cr);
    hipLaunchKernelGGL(k_eval_nn, dim3(nblk), dim3(64), 0, stream, src_cu, ref_xyz, ref_cu, raw_xyz, raw_cu, nb,
                       l.blk_cu, l.A, l.Cr, status, d2_src, nn_src, d2_ref, nn_ref, l.part);
    hipLaunchKernelGGL(k_eval_finish, dim3(nb), dim3(64), 0, stream, src_cu, ref_cu, l.blk_cu, l.part, status, metrics);
  }
  SPR_LAUNCH_CHECK();
  return 0;
}
