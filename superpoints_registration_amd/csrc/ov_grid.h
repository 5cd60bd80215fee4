// The per-cloud cell table of the exact nearest-neighbour operators (gt_overlap.hip, icp.hip): grid description,
// 32-byte records, the cell of a float64 coordinate, the grid that fits a cloud's share of the table and the
// nine-run neighbourhood.  The argument for the 27-cell neighbourhood and for the capacity rule is gt_overlap.hip's.
#pragma once
#include <rocprim/device/device_scan.hpp>

#include "spr_common.h"

namespace spr {

struct OvGrid {
  double mn[3];
  double inv_h;
  int dim[3];
  int off;  // first cell of this cloud in the table
};

struct alignas(32) OvRec {
  double x, y, z;
  int idx;  // local to the cloud
  int pad;
};

constexpr int kOvCellsPerPoint = 16;
constexpr int kOvCellsBase = 4096;
constexpr double kOvMaxCoord = 1073741824.0;  // 2^30 cells

static inline size_t ov_scan_temp_bytes(size_t n) {
  size_t b = 0;
  (void)rocprim::exclusive_scan(nullptr, b, (int*)nullptr, (int*)nullptr, 0, n > 0 ? n : 1, rocprim::plus<int>());
  return align_up(b, 256) + 256;
}

#ifdef __HIPCC__
// cell coordinate of p in a grid, clamped to [-2, 2^30] (so that the int conversion is defined)
__device__ __forceinline__ int ov_cell(double p, double mn, double inv_h) {
  double v = (p - mn) * inv_h;
  v = fmin(fmax(v, -2.0), kOvMaxCoord);
  return (int)floor(v);
}

__device__ __forceinline__ int ov_grid_cell(const OvGrid& g, int cx, int cy, int cz) {
  return g.off + (cz * g.dim[1] + cy) * g.dim[0] + cx;
}

// The grid of a cloud of n > 0 finite points with bounding box [mn, mx]: the finest edge >= h0 whose grid fits the
// cloud's share of the table, 16 n + 4096 cells (h -> inf gives 1 x 1 x 1).  off is left 0.  Returns false when the
// grid does not fit after all (not reachable for finite boxes; the grid is then ONE cell that every finite coordinate
// falls into, inv_h = 0).
__device__ __forceinline__ bool ov_fit_grid(const double* mn, const double* mx, int n, double h0, OvGrid& g) {
  const double budget = (double)kOvCellsPerPoint * (double)n + (double)kOvCellsBase;
  double h = h0;
  for (int it = 0; it < 4096; ++it) {
    const double inv = 1.0 / h;
    double cells = 1.0;
    for (int d = 0; d < 3; ++d) cells *= floor(fmin((mx[d] - mn[d]) * inv, kOvMaxCoord)) + 1.0;
    g.inv_h = inv;
    if (cells <= budget) break;
    h *= 1.25;
  }
  for (int d = 0; d < 3; ++d) {
    g.mn[d] = mn[d];
    g.dim[d] = ov_cell(mx[d], g.mn[d], g.inv_h) + 1;
  }
  if ((double)g.dim[0] * (double)g.dim[1] * (double)g.dim[2] > budget) {
    g.dim[0] = g.dim[1] = g.dim[2] = 1;
    g.inv_h = 0.0;
    return false;
  }
  return true;
}

struct OvRuns9 {
  int2 r0, r1, r2, r3, r4, r5, r6, r7, r8;
};
// a nine-element array indexed by the running run number would be demoted to scratch memory (radius_neighbors.hip)
__device__ __forceinline__ int2 ov_pick9(int k, const OvRuns9& a) {
  int2 v = a.r0;
  v = (k == 1) ? a.r1 : v;
  v = (k == 2) ? a.r2 : v;
  v = (k == 3) ? a.r3 : v;
  v = (k == 4) ? a.r4 : v;
  v = (k == 5) ? a.r5 : v;
  v = (k == 6) ? a.r6 : v;
  v = (k == 7) ? a.r7 : v;
  v = (k == 8) ? a.r8 : v;
  return v;
}

// The record runs of the 3 x 3 x 3 neighbourhood of cell (cx, cy, cz) in grid g: nine (begin, end) pairs into the
// record array, one per (z, y) row; a row outside the grid is the empty run (0, 0).
__device__ __forceinline__ OvRuns9 ov_runs(const OvGrid& g, const int* __restrict__ start, int cx, int cy, int cz) {
  const int xlo = max(cx - 1, 0), xhi = min(cx + 1, g.dim[0] - 1);
  auto run_of = [&](int k) -> int2 {
    const int z = cz + k / 3 - 1, y = cy + k % 3 - 1;
    const bool in = xlo <= xhi && z >= 0 && z < g.dim[2] && y >= 0 && y < g.dim[1];
    if (!in) return make_int2(0, 0);
    return make_int2(start[ov_grid_cell(g, xlo, y, z)], start[ov_grid_cell(g, xhi, y, z) + 1]);
  };
  OvRuns9 runs;
  runs.r0 = run_of(0); runs.r1 = run_of(1); runs.r2 = run_of(2);
  runs.r3 = run_of(3); runs.r4 = run_of(4); runs.r5 = run_of(5);
  runs.r6 = run_of(6); runs.r7 = run_of(7); runs.r8 = run_of(8);
  return runs;
}

// The nearest record of the nine runs to (x, y, z) under the lexicographic order (d2, index), d2 in float64 with one
// rounding per operation; only d2 < r2 (strict) counts.  The nine runs are walked as ONE candidate sequence, four
// 32-byte records in flight.  Returns the record's index or -1; best_d2 = its d2 (r2 when there is none).
__device__ __forceinline__ int ov_nearest(const OvRec* __restrict__ rec, const OvRuns9& runs, double x, double y,
                                          double z, double r2, double& best_d2) {
  double best = r2;  // strict: only d2 < r2 can replace it
  int best_i = -1;
  int k = 0, j = runs.r0.x, e = runs.r0.y;
  while (k < 9) {
    OvRec s4[4];
    bool v4[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      while (k < 9 && j >= e) {
        ++k;
        const int2 r = ov_pick9(k, runs);
        j = r.x;
        e = r.y;
      }
      v4[u] = k < 9;
      s4[u] = rec[v4[u] ? j : 0];
      j += v4[u] ? 1 : 0;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const double dx = __dsub_rn(x, s4[u].x), dy = __dsub_rn(y, s4[u].y), dz = __dsub_rn(z, s4[u].z);
      double d2 = __dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy));
      d2 = __dadd_rn(d2, __dmul_rn(dz, dz));
      // lexicographic (d2, index); best_i = -1 stands for (r2, +inf)
      const bool better = v4[u] && (d2 < best || (d2 == best && best_i >= 0 && s4[u].idx < best_i));
      best = better ? d2 : best;
      best_i = better ? s4[u].idx : best_i;
    }
  }
  best_d2 = best;
  return best_i;
}
#endif

}  // namespace spr
