// 8f-5 -- ground-truth overlap masks and mutual correspondences on gfx950.
//
// Behaviour contract: compute_overlap() of the reference (utils/pointcloud.py:8-65: one Open3D kd-tree radius
// query per point, nearest hit kept), written out as a float64 definition (Open3D itself is absent: parity with
// it is unpinned).  For one pair (src [N,3], tgt [M,3], pose [3,4] src -> tgt, radius), every
// operation in IEEE float64 on the exactly converted float32 inputs, one rounding per operation (no FMA):
//   s'_i[k]      = ((R[k][0] x + R[k][1] y) + R[k][2] z) + t[k]
//   d2(a, b)     = ((ax - bx)^2 + (ay - by)^2) + (az - bz)^2
//   src_corr[i]  = the j minimising (d2(s'_i, tgt_j), j) if that d2 < radius * radius (strict), else -1
//   tgt_corr[j]  = the i minimising (d2(tgt_j, s'_i), i), same rule
//   masks        = corr >= 0
//   corr [2, K]  = the pairs (i, src_corr[i]) with src_corr[i] > 0 and tgt_corr[src_corr[i]] == i, ascending i.
// The `> 0` (not `>= 0`) is the reference's (utils/pointcloud.py:57-58): a source point whose mutual partner is
// target index 0 is missing from the correspondence list while its mask bit is set.  Reproduced on purpose.
// Indices are local to the pair's clouds.  The result is a pure function of the inputs: integer / bool outputs
// identical to a numpy float64 evaluation of the rules above, whatever the batch composition.
//
// One call handles all B pairs, both directions:
//   the 2 B clouds [tgt_0 .. tgt_{B-1}, src'_0 .. src'_{B-1}] (sources TRANSFORMED) share one cell table --
//   k_ov_bbox     per cloud: float64 bounding box -> cell edge and grid dims
//   k_ov_offsets  prefix of the per-cloud cell counts, the combined cu array
//   k_ov_count    one integer atomic per point: cell population and arrival rank
//   rocPRIM exclusive scan -> cell starts
//   k_ov_scatter  counting-sort scatter of 32-byte records (float64 x y z, local index)
//   k_ov_scan     one thread per RECORD (queries walk in cell order: the lanes of a wave scan the same cells): the
//                 3 x 3 x 3 neighbourhood in the OTHER cloud of its pair is nine contiguous record runs; the
//                 running (d2, index) minimum stays in registers
//   k_ov_mark -> rocPRIM exclusive scan -> k_ov_compact: mutual test and ordered compaction.
//
// Cell assignment.  cell = floor((p - min) * (1 / h)) in float64 with h >= radius * (1 + 2^-8).  Two points with
// computed d2 < fl(radius^2) differ by at most radius (1 + 2^-51) per axis, i.e. by less than 1 - 2^-9 cells; the
// two roundings of the cell coordinate move it by < 2^-22 cells (coordinates are clamped below 2^30), so the floors
// differ by at most one: every partner lies in the 27-cell neighbourhood.  Each cloud has its OWN grid (its own
// bounding box); a query is located in the other cloud's grid with its coordinate clamped to [-2, 2^30] cells, so
// a query outside that box by more than a cell meets no cell at all -- clouds that do not overlap cost nothing and
// never enlarge a table.  The order inside a cell depends on atomic arrival order, the OUTPUT does not: the
// minimum over (d2, index) is order independent.
//
// Capacity.  A cloud of n points gets at most 16 n + 4096 cells: when its box needs more at h = radius (1 + 2^-8)
// the edge grows (x 1.25 per step) until it fits.  Coarser cells are as correct as fine ones (more candidates per
// query, same minimum), so no geometry overflows the table; only non-finite coordinates are refused
// (corr_count[0] = -1 -> ops raises).
//
// The grid description, the records, the grid fit and the nine-run walk live in ov_grid.h, shared with icp.hip.
#include "ov_grid.h"

namespace spr {
namespace {

// s' = ((R0 x + R1 y) + R2 z) + t, one rounding per operation
__device__ __forceinline__ void ov_transform(const float* __restrict__ T, float xf, float yf, float zf, double* o) {
  const double x = (double)xf, y = (double)yf, z = (double)zf;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    double a = __dadd_rn(__dmul_rn((double)T[4 * k + 0], x), __dmul_rn((double)T[4 * k + 1], y));
    a = __dadd_rn(a, __dmul_rn((double)T[4 * k + 2], z));
    o[k] = __dadd_rn(a, (double)T[4 * k + 3]);
  }
}

// point p of the combined sequence [all targets, all sources] of cloud c (c < nb: target of pair c, otherwise the
// TRANSFORMED source of pair c - nb)
__device__ __forceinline__ void ov_point(const float* __restrict__ src, const float* __restrict__ tgt,
                                         const float* __restrict__ pose, int nt, int nb, int c, int p, double* o) {
  if (c < nb) {
    o[0] = (double)tgt[3 * (size_t)p + 0];
    o[1] = (double)tgt[3 * (size_t)p + 1];
    o[2] = (double)tgt[3 * (size_t)p + 2];
  } else {
    const size_t g = (size_t)(p - nt);
    ov_transform(pose + 12 * (size_t)(c - nb), src[3 * g + 0], src[3 * g + 1], src[3 * g + 2], o);
  }
}

__global__ __launch_bounds__(256) void k_ov_bbox(const float* __restrict__ src, const int* __restrict__ src_cu,
                                                 const float* __restrict__ tgt, const int* __restrict__ tgt_cu,
                                                 const float* __restrict__ pose, int nt, int nb, double h0,
                                                 OvGrid* info, int* err) {
  const int c = blockIdx.x;
  const int beg = c < nb ? tgt_cu[c] : nt + src_cu[c - nb];
  const int end = c < nb ? tgt_cu[c + 1] : nt + src_cu[c - nb + 1];
  __shared__ double smn[3][256], smx[3][256];
  __shared__ int sbad;
  if (threadIdx.x == 0) sbad = 0;
  __syncthreads();
  double mn[3] = {1.0e300, 1.0e300, 1.0e300}, mx[3] = {-1.0e300, -1.0e300, -1.0e300};
  bool bad = false;
  for (int p = beg + threadIdx.x; p < end; p += blockDim.x) {
    double v[3];
    ov_point(src, tgt, pose, nt, nb, c, p, v);
    for (int d = 0; d < 3; ++d) {
      bad = bad || !(fabs(v[d]) < 1.0e300);
      mn[d] = fmin(mn[d], v[d]);
      mx[d] = fmax(mx[d], v[d]);
    }
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
  if (threadIdx.x != 0) return;
  OvGrid g;
  g.off = 0;
  g.inv_h = 1.0 / h0;
  for (int d = 0; d < 3; ++d) {
    g.mn[d] = 0.0;
    g.dim[d] = 1;
  }
  if (sbad) {
    atomicOr(err, 1);
  } else if (end > beg) {
    const double bmn[3] = {smn[0][0], smn[1][0], smn[2][0]}, bmx[3] = {smx[0][0], smx[1][0], smx[2][0]};
    if (!ov_fit_grid(bmn, bmx, end - beg, h0, g)) atomicOr(err, 1);  // not reachable for finite boxes
  }
  info[c] = g;
}

// ccu [2 nb + 1]: the combined sequence's cloud boundaries
__global__ void k_ov_offsets(OvGrid* info, const int* __restrict__ src_cu, const int* __restrict__ tgt_cu, int nt,
                             int nb, int* ccu) {
  for (int c = threadIdx.x; c <= nb; c += blockDim.x) {
    if (c < nb) ccu[c] = tgt_cu[c];
    ccu[nb + c] = nt + src_cu[c];
  }
  if (threadIdx.x != 0) return;
  int off = 0;
  for (int c = 0; c < 2 * nb; ++c) {
    info[c].off = off;
    off += info[c].dim[0] * info[c].dim[1] * info[c].dim[2];
  }
}

__global__ __launch_bounds__(256) void k_ov_count(const float* __restrict__ src, const float* __restrict__ tgt,
                                                  const float* __restrict__ pose, int nt, int np, int nb,
                                                  const int* __restrict__ ccu, const OvGrid* __restrict__ info,
                                                  const int* __restrict__ err, int* count, int* cell_of, int* rank) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= np || *err) return;
  const int c = find_segment(ccu, 2 * nb, p);
  const OvGrid g = info[c];
  double v[3];
  ov_point(src, tgt, pose, nt, nb, c, p, v);
  const int cx = min(max(ov_cell(v[0], g.mn[0], g.inv_h), 0), g.dim[0] - 1);
  const int cy = min(max(ov_cell(v[1], g.mn[1], g.inv_h), 0), g.dim[1] - 1);
  const int cz = min(max(ov_cell(v[2], g.mn[2], g.inv_h), 0), g.dim[2] - 1);
  const int L = ov_grid_cell(g, cx, cy, cz);
  cell_of[p] = L;
  rank[p] = atomicAdd(&count[L], 1);  // arrival rank inside the cell
}

__global__ __launch_bounds__(256) void k_ov_scatter(const float* __restrict__ src, const float* __restrict__ tgt,
                                                    const float* __restrict__ pose, int nt, int np, int nb,
                                                    const int* __restrict__ ccu, const int* __restrict__ err,
                                                    const int* __restrict__ cell_of, const int* __restrict__ start,
                                                    const int* __restrict__ rank, OvRec* rec) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= np || *err) return;
  const int c = find_segment(ccu, 2 * nb, p);
  double v[3];
  ov_point(src, tgt, pose, nt, nb, c, p, v);
  OvRec r;
  r.x = v[0], r.y = v[1], r.z = v[2];
  r.idx = p - ccu[c];
  r.pad = 0;
  rec[start[cell_of[p]] + rank[p]] = r;
}

// Thread t owns record t: a point of cloud c, looked up in the table of the other cloud of its pair.
__global__ __launch_bounds__(256) void k_ov_scan(int np, int nt, int nb, const int* __restrict__ ccu,
                                                 const OvGrid* __restrict__ info, const int* __restrict__ start,
                                                 const OvRec* __restrict__ rec, const int* __restrict__ err, double r2,
                                                 int* __restrict__ src_corr, int* __restrict__ tgt_corr,
                                                 unsigned char* __restrict__ src_mask,
                                                 unsigned char* __restrict__ tgt_mask) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= np || *err) return;
  const int c = find_segment(ccu, 2 * nb, t);
  const OvGrid g = info[c < nb ? c + nb : c - nb];
  const OvRec me = rec[t];
  const int cx = ov_cell(me.x, g.mn[0], g.inv_h);
  const int cy = ov_cell(me.y, g.mn[1], g.inv_h);
  const int cz = ov_cell(me.z, g.mn[2], g.inv_h);
  double best;
  const int best_i = ov_nearest(rec, ov_runs(g, start, cx, cy, cz), me.x, me.y, me.z, r2, best);
  // rows are addressed by the point's ORIGINAL index, not by its place in the cell order
  if (c < nb) {
    const int o = ccu[c] + me.idx;
    tgt_corr[o] = best_i;
    tgt_mask[o] = best_i >= 0 ? 1 : 0;
  } else {
    const int o = ccu[c] - nt + me.idx;
    src_corr[o] = best_i;
    src_mask[o] = best_i >= 0 ? 1 : 0;
  }
}

// flag[i] = source point i (global) has a mutual partner other than target 0; flag[ns] = 0
__global__ __launch_bounds__(256) void k_ov_mark(int ns, int nb, const int* __restrict__ src_cu,
                                                 const int* __restrict__ tgt_cu, const int* __restrict__ err,
                                                 const int* __restrict__ src_corr, const int* __restrict__ tgt_corr,
                                                 int* flag) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > ns) return;
  int f = 0;
  if (i < ns && !*err) {
    const int c = find_segment(src_cu, nb, i);
    const int j = src_corr[i];
    if (j > 0) f = tgt_corr[tgt_cu[c] + j] == i - src_cu[c] ? 1 : 0;  // `> 0`: utils/pointcloud.py:57-58
  }
  flag[i] = f;
}

// pair c's correspondences go to columns [src_cu[c], src_cu[c] + corr_count[c]) of corr [2, ns], ascending i
__global__ __launch_bounds__(256) void k_ov_compact(int ns, int nb, const int* __restrict__ src_cu,
                                                    const int* __restrict__ err, const int* __restrict__ src_corr,
                                                    const int* __restrict__ flag, const int* __restrict__ pos,
                                                    int* __restrict__ corr, int* __restrict__ corr_count) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nb) corr_count[i] = *err ? -1 : pos[src_cu[i + 1]] - pos[src_cu[i]];
  if (i >= ns || *err || !flag[i]) return;
  const int c = find_segment(src_cu, nb, i);
  const int b = src_cu[c];
  const int o = b + (pos[i] - pos[b]);
  corr[o] = i - b;
  corr[(size_t)ns + o] = src_corr[i];
}

size_t ov_cells(int ns, int nt, int nb) {
  return (size_t)kOvCellsPerPoint * ((size_t)ns + (size_t)nt) + (size_t)kOvCellsBase * 2 * (size_t)nb;
}

struct OvWs {
  OvGrid* info;
  int *ccu, *err, *count, *start, *cell_of, *rank;
  OvRec* rec;
  int *flag, *pos;
  void* temp;
  size_t cells, temp_bytes;
};
OvWs ov_layout(Workspace& w, int ns, int nt, int nb) {
  OvWs l;
  const size_t np = (size_t)ns + (size_t)nt, B = nb > 0 ? nb : 1;   // the query measures nb = 0 as one pair
  l.cells = ov_cells(ns, nt, nb);
  l.info = w.take<OvGrid>(2 * B);
  l.ccu = w.take<int>(2 * B + 1);
  l.err = w.take<int>(64);
  l.count = w.take<int>(l.cells + 1);
  l.start = w.take<int>(l.cells + 1);
  l.cell_of = w.take<int>(np > 0 ? np : 1);
  l.rank = w.take<int>(np > 0 ? np : 1);
  l.rec = w.take<OvRec>(np > 0 ? np : 1);
  l.flag = w.take<int>((size_t)ns + 1);
  l.pos = w.take<int>((size_t)ns + 1);
  l.temp_bytes = ov_scan_temp_bytes(l.cells + 1 > (size_t)ns + 1 ? l.cells + 1 : (size_t)ns + 1);
  l.temp = w.take<char>(l.temp_bytes);
  return l;
}

}  // namespace
}  // namespace spr

using namespace spr;

extern "C" size_t spr_gt_overlap_workspace_bytes(int ns, int nt, int nb) {
  if (ns < 0 || nt < 0 || nb < 0) return 0;
  return measure(ov_layout, ns, nt, nb);
}

extern "C" int spr_gt_overlap(const float* src_xyz, const int* src_cu, int ns, const float* tgt_xyz,
                              const int* tgt_cu, int nt, const float* pose, int nb, double radius, int* src_corr,
                              int* tgt_corr, unsigned char* src_mask, unsigned char* tgt_mask, int* corr,
                              int* corr_count, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPR_REQUIRE(nb >= 0 && ns >= 0 && nt >= 0, "gt_overlap: negative size (nb=%d ns=%d nt=%d)", nb, ns, nt);
  SPR_REQUIRE(radius > 0.0 && radius < 1.0e150, "gt_overlap: radius must be > 0 (and finite), got %g", radius);
  SPR_REQUIRE(nb < 32768, "gt_overlap: at most 32767 pairs per call");
  SPR_REQUIRE((size_t)ns + (size_t)nt <= ((size_t)1 << 26), "gt_overlap: at most 2^26 points per call");
  SPR_REQUIRE(nb > 0 || (ns == 0 && nt == 0), "gt_overlap: points without pairs (nb=0 ns=%d nt=%d)", ns, nt);
  if (nb == 0) return 0;
  SPR_REQUIRE(src_cu && tgt_cu && pose && corr_count, "gt_overlap: src_cu, tgt_cu, pose and corr_count must not be null");
  SPR_REQUIRE(ns == 0 || (src_xyz && src_corr && src_mask && corr), "gt_overlap: null source pointer with ns=%d", ns);
  SPR_REQUIRE(nt == 0 || (tgt_xyz && tgt_corr && tgt_mask), "gt_overlap: null target pointer with nt=%d", nt);
  Workspace w(ws, ws_bytes);
  const auto [info, ccu, err, count, start, cell_of, rank, rec, flag, pos, temp, cells, temp_bytes] = ov_layout(w, ns, nt, nb);
  SPR_REQUIRE(ws != nullptr && w.ok(), "gt_overlap: workspace too small");
  const int np = ns + nt;

  const double h0 = radius * (1.0 + 1.0 / 256.0);
  const double r2 = radius * radius;
  const int TB = 256;
  SPR_HIP_CHECK(hipMemsetAsync(err, 0, 64 * sizeof(int), stream));
  SPR_HIP_CHECK(hipMemsetAsync(count, 0, (cells + 1) * sizeof(int), stream));
  hipLaunchKernelGGL(k_ov_bbox, dim3(2 * nb), dim3(256), 0, stream, src_xyz, src_cu, tgt_xyz, tgt_cu, pose, nt, nb, h0,
                     info, err);
  hipLaunchKernelGGL(k_ov_offsets, dim3(1), dim3(256), 0, stream, info, src_cu, tgt_cu, nt, nb, ccu);
  if (np > 0) {
    hipLaunchKernelGGL(k_ov_count, dim3(cdiv(np, TB)), dim3(TB), 0, stream, src_xyz, tgt_xyz, pose, nt, np, nb, ccu, info,
                       err, count, cell_of, rank);
    SPR_LAUNCH_CHECK();
    size_t tb = temp_bytes;
    SPR_HIP_CHECK(rocprim::exclusive_scan(temp, tb, count, start, 0, cells + 1, rocprim::plus<int>(), stream));
    hipLaunchKernelGGL(k_ov_scatter, dim3(cdiv(np, TB)), dim3(TB), 0, stream, src_xyz, tgt_xyz, pose, nt, np, nb, ccu,
                       err, cell_of, start, rank, rec);
    hipLaunchKernelGGL(k_ov_scan, dim3(cdiv(np, TB)), dim3(TB), 0, stream, np, nt, nb, ccu, info, start, rec, err, r2,
                       src_corr, tgt_corr, src_mask, tgt_mask);
  }
  hipLaunchKernelGGL(k_ov_mark, dim3(cdiv(ns + 1, TB)), dim3(TB), 0, stream, ns, nb, src_cu, tgt_cu, err, src_corr,
                     tgt_corr, flag);
  SPR_LAUNCH_CHECK();
  size_t tb = temp_bytes;
  SPR_HIP_CHECK(rocprim::exclusive_scan(temp, tb, flag, pos, 0, (size_t)ns + 1, rocprim::plus<int>(), stream));
  hipLaunchKernelGGL(k_ov_compact, dim3(cdiv(ns > nb ? ns : nb, TB)), dim3(TB), 0, stream, ns, nb, src_cu, err, src_corr,
                     flag, pos, corr, corr_count);
  SPR_LAUNCH_CHECK();
  return 0;
}
