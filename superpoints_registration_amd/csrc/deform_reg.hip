// The regulariser of deformable KPConv on gfx950: KPConv's fitting and repulsive losses on the deformed kernel points,
// value and gradient at the offset features in ONE launch.
//
// Contract (include/spr.h, spr_deform_reg), with K kernel points kp, extent e, offset features of and R = repulse_extent:
//     D[n,p]  = kp[p] + e of[n, 3p:3p+3]                   (float32, the arithmetic of k_kpconv_deform_min_d2)
//     y[n,k]  = s[idx[n,k]] - q[n]                         real entries only (an index outside [0, ns) is a shadow)
//     m[n,p]  = min over real k of |y[n,k] - D[n,p]|^2,  k* the lowest column that attains it; no real entry: m = 0
//     fit     = sum m / e^2 / (nq K);   L = D / e;   rep = sum_n sum_i sum_{j != i} min(|L_i - L_j| - R, 0)^2 / (nq K)
//     value   = 2 fit + rep
//     d value / d of[n, 3p:3p+3] = [4 (D[n,p] - y[n,k*]) / e + 2 sum_{j != p} min(dist - R, 0) (L_p - L_j) / dist] / (nq K)
//     d value / d of[n, 3K + p]  = 0;  a pair with dist == 0 contributes no gradient; the other points are constants
//
// k_deform_reg<GRAD>: one 16-lane group per query, lane = kernel point, four queries per wave, 16 per workgroup.  The
//   16 lanes of a group share the row: lane l loads the columns k = l (mod 16) once (index, support point, difference
//   to the query) and the group reads them from each other with __shfl -- one gather per (query, column) where
//   k_kpconv_deform_min_d2 does one per (query, column, kernel point).  The repulsive term reads the other lanes' L the
//   same way.  k* and the pair geometry are in registers when the value is known, so the gradient row is written by the
//   same launch (GRAD; the validation instance stores nothing but its partials).  Every lane of a group stays alive for
//   the shuffles: rows past nq and lanes past K load clamped addresses and contribute nothing.
//   The workgroup's two sums are float64 (block_sum_d: wave sums, waves in ascending order) -> part[2 blockIdx.x + {0,1}].
// k_deform_reg_final: one workgroup adds the partials in a fixed order (thread t takes blocks t, t + 256, ...; then
//   block_sum_d) -> out[3] = (value, fit, rep) as float32.  No atomics anywhere: two runs give the same bits.
#include "spr_common.h"
#include "kpconv_walk.h"

namespace spr {
namespace {

constexpr int kGroup = 16;               // lanes per query = kernel points at most
constexpr int kQPB = 256 / kGroup;       // queries per workgroup
static_assert(kGroup == kWalkKP, "one lane per kernel point");

template <bool GRAD>
__global__ __launch_bounds__(256) void k_deform_reg(const float* __restrict__ q_xyz, int nq,
                                                    const float* __restrict__ s_xyz, int ns,
                                                    const int* __restrict__ nbr, int nbr_stride, int kmax,
                                                    const float* __restrict__ kpts, int n_kp, float extent,
                                                    const float* __restrict__ of, int of_stride, int od, float repulse,
                                                    float grad_scale, double* __restrict__ part,
                                                    float* __restrict__ d_of) {
  __shared__ double sh[4];
  const int p = threadIdx.x & (kGroup - 1);
  const int n = blockIdx.x * kQPB + (threadIdx.x >> 4);
  const bool row = n < nq;
  const bool live = row && p < n_kp;
  const size_t nc = (size_t)(row ? n : nq - 1);
  const int pc = p < n_kp ? p : n_kp - 1;
  const float qx = q_xyz[3 * nc], qy = q_xyz[3 * nc + 1], qz = q_xyz[3 * nc + 2];
  const float* o = of + nc * of_stride;
  const float Dx = kpts[3 * pc] + extent * o[3 * pc], Dy = kpts[3 * pc + 1] + extent * o[3 * pc + 1],
              Dz = kpts[3 * pc + 2] + extent * o[3 * pc + 2];

  // ---- fitting term: the nearest real neighbour of D, lowest column first --------------------------------------------
  float best = __builtin_inff(), bx = 0.f, by = 0.f, bz = 0.f;   // b = y[k*] - D
  const int* idx_row = nbr + nc * nbr_stride;
  for (int kb = 0; kb < kmax; kb += kGroup) {
    const int k = kb + p;
    int ok = 0;
    float yx = 0.f, yy = 0.f, yz = 0.f;
    if (row && k < kmax) {
      const int idx = idx_row[k];
      if (idx >= 0 && idx < ns) {
        ok = 1;
        yx = s_xyz[3 * (size_t)idx] - qx;
        yy = s_xyz[3 * (size_t)idx + 1] - qy;
        yz = s_xyz[3 * (size_t)idx + 2] - qz;
      }
    }
    const int jn = min(kGroup, kmax - kb);   // uniform
    for (int j = 0; j < jn; ++j) {
      const int okj = __shfl(ok, j, kGroup);
      const float dx = __shfl(yx, j, kGroup) - Dx, dy = __shfl(yy, j, kGroup) - Dy, dz = __shfl(yz, j, kGroup) - Dz;
      const float d2 = dx * dx + dy * dy + dz * dz;
      if (okj && d2 < best) {
        best = d2;
        bx = dx;
        by = dy;
        bz = dz;
      }
    }
  }
  const bool found = best < __builtin_inff();

  // ---- repulsive term: the other kernel points of the query, as constants ------------------------------------------------
  const float Lx = Dx / extent, Ly = Dy / extent, Lz = Dz / extent;
  float rep = 0.f, rx = 0.f, ry = 0.f, rz = 0.f;
  for (int j = 0; j < n_kp; ++j) {
    const float ex = Lx - __shfl(Lx, j, kGroup), ey = Ly - __shfl(Ly, j, kGroup), ez = Lz - __shfl(Lz, j, kGroup);
    const float dist = sqrtf(ex * ex + ey * ey + ez * ez);
    const float h = j != p ? fminf(dist - repulse, 0.f) : 0.f;
    rep += h * h;
    if (GRAD && dist > 0.f) {   // dist == 0 (the point itself, or a coincident one): no gradient
      const float c = h / dist;
      rx += c * ex;
      ry += c * ey;
      rz += c * ez;
    }
  }

  const double fit_sum = block_sum_d(live && found ? (double)best : 0.0, sh);
  const double rep_sum = block_sum_d(live ? (double)rep : 0.0, sh);
  if (threadIdx.x == 0) {
    part[2 * (size_t)blockIdx.x] = fit_sum;
    part[2 * (size_t)blockIdx.x + 1] = rep_sum;
  }
  if (GRAD && live) {
    const float f = found ? 4.f / extent : 0.f;   // D - y[k*] = -b
    float* g = d_of + (size_t)n * od;
    g[3 * p] = grad_scale * (2.f * rx - f * bx);
    g[3 * p + 1] = grad_scale * (2.f * ry - f * by);
    g[3 * p + 2] = grad_scale * (2.f * rz - f * bz);
    if (od > 3 * n_kp) g[3 * n_kp + p] = 0.f;
  }
}

__global__ __launch_bounds__(256) void k_deform_reg_final(const double* __restrict__ part, int nblocks, double fit_scale,
                                                          double rep_scale, float* __restrict__ out) {
  __shared__ double sh[4];
  double f = 0.0, r = 0.0;
  for (int b = threadIdx.x; b < nblocks; b += 256) {
    f += part[2 * (size_t)b];
    r += part[2 * (size_t)b + 1];
  }
  const double fit = block_sum_d(f, sh) * fit_scale;
  const double rep = block_sum_d(r, sh) * rep_scale;
  if (threadIdx.x == 0) {
    out[0] = (float)(2.0 * fit + rep);
    out[1] = (float)fit;
    out[2] = (float)rep;
  }
}

struct RegWs {
  double* part;   // [workgroups][2]
};
RegWs reg_layout(Workspace& w, int nq) {
  RegWs l;
  l.part = nq > 0 ? w.take<double>(2 * (size_t)cdiv(nq, kQPB)) : nullptr;
  return l;
}

}  // namespace
}  // namespace spr

using namespace spr;

extern "C" size_t spr_deform_reg_workspace_size(int nq) { return measure(reg_layout, nq); }

extern "C" int spr_deform_reg(const float* q_xyz, int nq, const float* s_xyz, int ns, const int* nbr, int nbr_stride,
                              int kmax, const float* kernel_points, int n_kp, float kp_extent,
                              const float* offset_features, int of_stride, int modulated, float repulse_extent,
                              float* out, float* d_offset_features, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPR_REQUIRE(nq > 0 && ns > 0, "deform_reg: empty input");
  SPR_REQUIRE(kmax >= 1 && kmax <= nbr_stride, "deform_reg: bad kmax=%d stride=%d", kmax, nbr_stride);
  SPR_REQUIRE(n_kp >= 1 && n_kp <= kGroup, "deform_reg: %d kernel points (at most %d)", n_kp, kGroup);
  SPR_REQUIRE(kp_extent > 0.f, "deform_reg: KP_extent must be > 0");
  SPR_REQUIRE(repulse_extent >= 0.f, "deform_reg: repulse_extent must be >= 0");
  SPR_REQUIRE(modulated == 0 || modulated == 1, "deform_reg: modulated is 0 or 1");
  SPR_REQUIRE(offset_features != nullptr && of_stride >= (3 + modulated) * n_kp,
              "deform_reg: offset features need %d columns, row stride %d", (3 + modulated) * n_kp, of_stride);
  Workspace w(ws, ws_bytes);
  const RegWs l = reg_layout(w, nq);
  SPR_REQUIRE(ws != nullptr && w.ok(), "deform_reg: workspace too small");
  SPR_REQUIRE(q_xyz != nullptr && s_xyz != nullptr && nbr != nullptr && kernel_points != nullptr && out != nullptr,
              "deform_reg: null argument");
  const int nblocks = cdiv(nq, kQPB);
  const int od = (3 + modulated) * n_kp;
  const double count = (double)nq * (double)n_kp;
  const float grad_scale = (float)(1.0 / count);
  if (d_offset_features != nullptr) {
    hipLaunchKernelGGL((k_deform_reg<true>), dim3(nblocks), dim3(256), 0, stream, q_xyz, nq, s_xyz, ns, nbr, nbr_stride,
                       kmax, kernel_points, n_kp, kp_extent, offset_features, of_stride, od, repulse_extent, grad_scale,
                       l.part, d_offset_features);
  } else {
    hipLaunchKernelGGL((k_deform_reg<false>), dim3(nblocks), dim3(256), 0, stream, q_xyz, nq, s_xyz, ns, nbr,
                       nbr_stride, kmax, kernel_points, n_kp, kp_extent, offset_features, of_stride, od, repulse_extent,
                       grad_scale, l.part, (float*)nullptr);
  }
  SPR_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_deform_reg_final, dim3(1), dim3(256), 0, stream, (const double*)l.part, nblocks,
                     1.0 / ((double)kp_extent * (double)kp_extent * count), 1.0 / count, out);
  SPR_LAUNCH_CHECK();
  return 0;
}
