// Circle feature loss (feature_loss_type: circle) forward and backward on gfx950.
//
// Behaviour contract (reference source tree):
//   CircleLossFull(dist_type='euclidean')     models/losses/feature_loss.py:160-243
//   selected by qk_regtr_full.py:91-96; the Predator / D3Feat circle loss.
// Per pair, a = source features [N, D], b = target features [M, D], xa = source keypoints
// transformed by pose_gt, xb = target keypoints:
//   cd = ||xa_i - xb_j||,  fd = sqrt(sum_k (a_ik - b_jk)^2 + 1e-12)
//   pos = cd < r_p, neg = cd > r_n; a row / column is selected if it has a pos and a neg entry
//   lp = 10 (fd - 0.1) max(fd - 0.1, 0) on pos entries, ln = 10 (1.4 - fd) max(1.4 - fd, 0) on neg
//   entries; EVERY other entry has logit 0 and adds exp(0) = 1 to its logsumexp (the reference
//   masks with +-1e5 and then multiplies by a clamped weight of 0, so masked logits are 0, not -inf)
//   loss_row = softplus(lse_p_row + lse_n_row) / 10, loss_col likewise over columns
//   pair = (mean(loss_row[row_sel]) + mean(loss_col[col_sel])) / 2   (empty selection -> NaN)
//
// Structure.  All pairs of a step go through the same launches (grid.y = pair):
//   k_circle_tile   one 64 x 64 tile of (row, column) entries: fd by direct differences in f32 from
//                   32-wide D slabs of a and b staged in LDS (slab sums added in f64) (never the |a|^2 + |b|^2 - 2ab expansion:
//                   at |a| ~ 20 it cancels the fd < 1.4 region that decides the negative side); the
//                   tile's logits go to LDS and each row / column is reduced to (max, sum exp(l - max),
//                   has-pos / has-neg flags) per tile -- written as partials, no atomics
//   k_circle_lse    one thread per row / column: merges its tiles' partials in tile order in float64
//   k_circle_pair   one workgroup per pair: fixed-order float64 means over the selected rows / columns
// Backward (weights detached as in the reference): d loss / d fd_ij = c_i (sm_p,ij wp - sm_n,ij wn) +
// (same over column j), c = 0.5 / #selected * softplus'(s) * gout.  k_circle_grad recomputes the tile
// (same code, same bits) and writes G = (d loss / d fd) / fd into a dense [pair, max_n, max_m] matrix
// plus per-tile row / column sums of G; k_circle_gfinish merges those and initialises
// d_src = rowsum(G) a, d_tgt = colsum(G) b.  The caller finishes with two spr_bgemm calls
// (d_src -= G b, d_tgt -= G^T a).  Every sum has a fixed order: two calls give the same bits.
#include <cstdint>

#include "spr_common.h"

namespace spr {
namespace {

constexpr int CT = 64;        // tile edge (rows and columns)
constexpr int CK = 32;        // D slab staged in LDS
constexpr int LDT = CT + 1;   // padded LDS row
constexpr int CB = 256;       // threads per tile workgroup

// torch.nn.functional.softplus (beta 1, threshold 20) and its derivative
__device__ __forceinline__ double softplus_d(double s) { return s > 20.0 ? s : log1p(exp(s)); }
__device__ __forceinline__ double softplus_grad_d(double s) { return s > 20.0 ? 1.0 : 1.0 / (1.0 + exp(-s)); }

// keypoints transformed by the pair's ground-truth pose (se3_torch.py:16-35)
__global__ void k_circle_transform(const float* __restrict__ pose, const float* __restrict__ xyz,
                                   const int* __restrict__ cu, float* __restrict__ out) {
  const int b = blockIdx.y;
  const int r0 = cu[b], n = cu[b + 1] - r0;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* p = pose + 12 * b;
  const float* q = xyz + 3 * (size_t)(r0 + i);
  const float x = q[0], y = q[1], z = q[2];
#pragma unroll
  for (int r = 0; r < 3; ++r)
    out[3 * (size_t)(r0 + i) + r] = (x * p[4 * r] + y * p[4 * r + 1] + z * p[4 * r + 2]) + p[4 * r + 3];
}

struct TileGeom {
  int b, ra, ca, n, m, i0, j0, rows, cols;   // pair, its first global row / col, sizes, tile origin, valid extent
};

__device__ __forceinline__ bool tile_geom(const int* cu_a, const int* cu_b, int tiles_m_max, TileGeom& g) {
  g.b = blockIdx.y;
  g.ra = cu_a[g.b];
  g.ca = cu_b[g.b];
  g.n = cu_a[g.b + 1] - g.ra;
  g.m = cu_b[g.b + 1] - g.ca;
  g.i0 = (blockIdx.x / tiles_m_max) * CT;
  g.j0 = (blockIdx.x % tiles_m_max) * CT;
  if (g.i0 >= g.n || g.j0 >= g.m) return false;
  g.rows = min(CT, g.n - g.i0);
  g.cols = min(CT, g.m - g.j0);
  return true;
}

// fd and the pos / neg masks of the tile entries (ty + 16 r, tx + 16 c) owned by this thread.
// smem: >= 2 CK LDT floats (the a and b slabs, k-major).  d % 4 == 0.
__device__ __forceinline__ void fd_tile(const float* __restrict__ a, const float* __restrict__ bf, int d,
                                        const float* __restrict__ axyz, const float* __restrict__ bxyz,
                                        const TileGeom& g, float r_p, float r_n, float* smem, float fd[4][4],
                                        unsigned msk[4][4]) {
  float* As = smem;              // [k][row]
  float* Bs = smem + CK * LDT;   // [k][col]
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  // each 32-wide slab sums in f32, the slab sums in f64: the logits (~10 fd^2, thousands at LayerNorm scale)
  // magnify fd's relative error ~500-fold, so the 256-term f32 sum alone costs ~1e-4 in the softmax weights
  double accd[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) accd[r][c] = 0.0;
  // loader: 64 rows x 32 k = 512 float4 per operand, two per thread
  const int lr = tid >> 3, lk = (tid & 7) * 4;
  for (int k0 = 0; k0 < d; k0 += CK) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int row = lr + 32 * h;
      const int k = k0 + lk;
      float4 va = make_float4(0.f, 0.f, 0.f, 0.f), vb = va;
      if (k < d && row < g.rows) va = *(const float4*)(a + (size_t)(g.ra + g.i0 + row) * d + k);
      if (k < d && row < g.cols) vb = *(const float4*)(bf + (size_t)(g.ca + g.j0 + row) * d + k);
      As[(lk + 0) * LDT + row] = va.x;
      As[(lk + 1) * LDT + row] = va.y;
      As[(lk + 2) * LDT + row] = va.z;
      As[(lk + 3) * LDT + row] = va.w;
      Bs[(lk + 0) * LDT + row] = vb.x;
      Bs[(lk + 1) * LDT + row] = vb.y;
      Bs[(lk + 2) * LDT + row] = vb.z;
      Bs[(lk + 3) * LDT + row] = vb.w;
    }
    __syncthreads();
    float acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[r][c] = 0.f;
#pragma unroll 8
    for (int k = 0; k < CK; ++k) {
      float av[4], bv[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) av[r] = As[k * LDT + ty + 16 * r];
#pragma unroll
      for (int c = 0; c < 4; ++c) bv[c] = Bs[k * LDT + tx + 16 * c];
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float t = av[r] - bv[c];
          acc[r][c] = fmaf(t, t, acc[r][c]);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) accd[r][c] += (double)acc[r][c];
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = min(ty + 16 * r, g.rows - 1);
    const float* pa = axyz + 3 * (size_t)(g.ra + g.i0 + i);
    const float ax = pa[0], ay = pa[1], az = pa[2];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int j = min(tx + 16 * c, g.cols - 1);
      const float* pb = bxyz + 3 * (size_t)(g.ca + g.j0 + j);
      const float dx = ax - pb[0], dy = ay - pb[1], dz = az - pb[2];
      const float cd = sqrtf(dx * dx + dy * dy + dz * dz);
      fd[r][c] = (float)sqrt(accd[r][c] + 1e-12);
      msk[r][c] = (cd < r_p ? 1u : 0u) | (cd > r_n ? 2u : 0u);
    }
  }
}

// positive / negative logits and their (detached) weights of one entry
__device__ __forceinline__ void logits(float fd, unsigned msk, float& lp, float& wp, float& ln, float& wn) {
  const float tp = fd - 0.1f, tn = 1.4f - fd;
  wp = (msk & 1u) ? fmaxf(tp, 0.f) : 0.f;
  wn = (msk & 2u) ? fmaxf(tn, 0.f) : 0.f;
  lp = 10.f * tp * wp;
  ln = 10.f * tn * wn;
}

// Forward partials.  part[(row * tiles + t) * 2 + {0: pos, 1: neg}] = (max, sum exp(l - max)) over the
// tile's valid entries of that row (column); flag = has-pos | has-neg << 1.
__global__ __launch_bounds__(CB) void k_circle_tile(const float* __restrict__ a, const float* __restrict__ bf, int d,
                                                    const float* __restrict__ axyz, const float* __restrict__ bxyz,
                                                    const int* __restrict__ cu_a, const int* __restrict__ cu_b,
                                                    int tiles_n_max, int tiles_m_max, float r_p, float r_n,
                                                    float2* __restrict__ rpart, unsigned char* __restrict__ rflag,
                                                    float2* __restrict__ cpart, unsigned char* __restrict__ cflag) {
  __shared__ float smem[2 * CT * LDT];
  __shared__ unsigned char Ms[CT * LDT];
  TileGeom g;
  if (!tile_geom(cu_a, cu_b, tiles_m_max, g)) return;
  float fd[4][4];
  unsigned msk[4][4];
  fd_tile(a, bf, d, axyz, bxyz, g, r_p, r_n, smem, fd, msk);
  float* LP = smem;
  float* LN = smem + CT * LDT;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float lp, wp, ln, wn;
      logits(fd[r][c], msk[r][c], lp, wp, ln, wn);
      const int o = (ty + 16 * r) * LDT + tx + 16 * c;
      LP[o] = lp;
      LN[o] = ln;
      Ms[o] = (unsigned char)msk[r][c];
    }
  __syncthreads();
  const int grp = tid >> 6, x = tid & 63;
  const bool is_row = grp < 2;
  const int side = grp & 1;                       // 0: positive, 1: negative
  const float* L = side ? LN : LP;
  const int len = is_row ? g.cols : g.rows;
  if (x >= (is_row ? g.rows : g.cols)) return;
  const int st = is_row ? 1 : LDT, base = is_row ? x * LDT : x;
  float mx = -INFINITY;
  unsigned f = 0;
  for (int e = 0; e < len; ++e) {
    mx = fmaxf(mx, L[base + e * st]);
    f |= Ms[base + e * st];
  }
  float s = 0.f;
  for (int e = 0; e < len; ++e) s += expf(L[base + e * st] - mx);
  if (is_row) {
    const size_t o = (size_t)(g.ra + g.i0 + x) * tiles_m_max + g.j0 / CT;
    rpart[2 * o + side] = make_float2(mx, s);
    if (side == 0) rflag[o] = (unsigned char)f;
  } else {
    const size_t o = (size_t)(g.ca + g.j0 + x) * tiles_n_max + g.i0 / CT;
    cpart[2 * o + side] = make_float2(mx, s);
    if (side == 0) cflag[o] = (unsigned char)f;
  }
}

// lse[row] = (lse_p, lse_n) merged over the row's tiles in tile order (float64); sel[row] = has pos && has neg.
// blockIdx.z = 0: source rows (tiles over the target), 1: target columns (tiles over the source).
__global__ void k_circle_lse(const int* __restrict__ cu_a, const int* __restrict__ cu_b, int tiles_n_max,
                             int tiles_m_max, const float2* __restrict__ rpart, const unsigned char* __restrict__ rflag,
                             const float2* __restrict__ cpart, const unsigned char* __restrict__ cflag,
                             double2* __restrict__ rlse, int* __restrict__ rsel, double2* __restrict__ clse,
                             int* __restrict__ csel) {
  const int b = blockIdx.y;
  const bool col = blockIdx.z == 1;
  const int* cu = col ? cu_b : cu_a;
  const int* cv = col ? cu_a : cu_b;
  const int r0 = cu[b], n = cu[b + 1] - r0;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int nt = (cv[b + 1] - cv[b] + CT - 1) / CT, stride = col ? tiles_n_max : tiles_m_max;
  const float2* part = (col ? cpart : rpart) + 2 * (size_t)(r0 + i) * stride;
  const unsigned char* flag = (col ? cflag : rflag) + (size_t)(r0 + i) * stride;
  double lse[2];
  for (int side = 0; side < 2; ++side) {
    double mx = -INFINITY;
    for (int t = 0; t < nt; ++t) mx = fmax(mx, (double)part[2 * t + side].x);
    double s = 0.0;
    for (int t = 0; t < nt; ++t) s += (double)part[2 * t + side].y * exp((double)part[2 * t + side].x - mx);
    lse[side] = mx + log(s);
  }
  unsigned f = 0;
  for (int t = 0; t < nt; ++t) f |= flag[t];
  (col ? clse : rlse)[r0 + i] = make_double2(lse[0], lse[1]);
  (col ? csel : rsel)[r0 + i] = f == 3u;
}

// out[b] = (mean_sel softplus(s_row) / 10 + mean_sel softplus(s_col) / 10) / 2, float64 in a fixed order.
// With gout: coefficient of every row / column, coef = sel * gout[b] * 0.5 / #sel * softplus'(s).
__global__ __launch_bounds__(CB) void k_circle_pair(const int* __restrict__ cu_a, const int* __restrict__ cu_b,
                                                    const double2* __restrict__ rlse, const int* __restrict__ rsel,
                                                    const double2* __restrict__ clse, const int* __restrict__ csel,
                                                    float* __restrict__ out, const float* __restrict__ gout,
                                                    float* __restrict__ rcoef, float* __restrict__ ccoef) {
  __shared__ double sh[CB / 64];
  const int b = blockIdx.x;
  double mean[2], cnt[2];
  for (int side = 0; side < 2; ++side) {
    const int* cu = side ? cu_b : cu_a;
    const double2* lse = side ? clse : rlse;
    const int* sel = side ? csel : rsel;
    const int r0 = cu[b], n = cu[b + 1] - r0;
    double v = 0.0, c = 0.0;
    for (int i = threadIdx.x; i < n; i += CB)
      if (sel[r0 + i]) {
        v += softplus_d(lse[r0 + i].x + lse[r0 + i].y) / 10.0;
        c += 1.0;
      }
    const double tv = block_sum_d(v, sh);
    cnt[side] = block_sum_d(c, sh);
    mean[side] = tv / cnt[side];   // 0 / 0 = NaN for an empty selection, like torch's empty mean
    if (gout) {
      const double scale = cnt[side] > 0.0 ? (double)gout[b] * 0.5 / cnt[side] : 0.0;
      float* coef = side ? ccoef : rcoef;
      for (int i = threadIdx.x; i < n; i += CB)
        coef[r0 + i] = sel[r0 + i] ? (float)(scale * softplus_grad_d(lse[r0 + i].x + lse[r0 + i].y)) : 0.f;
    }
  }
  if (out && threadIdx.x == 0) out[b] = (float)((mean[0] + mean[1]) * 0.5);
}

// G[b][i][j] = (d loss / d fd_ij) / fd_ij for the tile (row stride max_m); per-tile row / column sums of G.
__global__ __launch_bounds__(CB) void k_circle_grad(const float* __restrict__ a, const float* __restrict__ bf, int d,
                                                    const float* __restrict__ axyz, const float* __restrict__ bxyz,
                                                    const int* __restrict__ cu_a, const int* __restrict__ cu_b,
                                                    int tiles_n_max, int tiles_m_max, float r_p, float r_n,
                                                    const double2* __restrict__ rlse, const float* __restrict__ rcoef,
                                                    const double2* __restrict__ clse, const float* __restrict__ ccoef,
                                                    int max_n, int max_m, float* __restrict__ G,
                                                    float* __restrict__ rgpart, float* __restrict__ cgpart) {
  __shared__ float smem[2 * CK * LDT];
  __shared__ double Rl[CT][2], Cl[CT][2];
  __shared__ float Rc[CT], Cc[CT];
  __shared__ float Cs[16][CT];
  TileGeom g;
  if (!tile_geom(cu_a, cu_b, tiles_m_max, g)) return;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  if (tid < CT) {
    const int i = min(tid, g.rows - 1);
    const double2 l = rlse[g.ra + g.i0 + i];
    Rl[tid][0] = l.x;
    Rl[tid][1] = l.y;
    Rc[tid] = tid < g.rows ? rcoef[g.ra + g.i0 + i] : 0.f;
  } else if (tid < 2 * CT) {
    const int x = tid - CT, j = min(x, g.cols - 1);
    const double2 l = clse[g.ca + g.j0 + j];
    Cl[x][0] = l.x;
    Cl[x][1] = l.y;
    Cc[x] = x < g.cols ? ccoef[g.ca + g.j0 + j] : 0.f;
  }
  float fd[4][4];
  unsigned msk[4][4];
  fd_tile(a, bf, d, axyz, bxyz, g, r_p, r_n, smem, fd, msk);   // its __syncthreads publish Rl .. Cc
  float rsum[4] = {0.f, 0.f, 0.f, 0.f}, csum[4] = {0.f, 0.f, 0.f, 0.f};
  float* Gb = G + (size_t)g.b * max_n * max_m;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = ty + 16 * r;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int j = tx + 16 * c;
      float lp, wp, ln, wn;
      logits(fd[r][c], msk[r][c], lp, wp, ln, wn);
      float gr = 0.f, gc = 0.f;
      if (Rc[i] != 0.f)
        gr = Rc[i] * (expf((float)((double)lp - Rl[i][0])) * wp - expf((float)((double)ln - Rl[i][1])) * wn);
      if (Cc[j] != 0.f)
        gc = Cc[j] * (expf((float)((double)lp - Cl[j][0])) * wp - expf((float)((double)ln - Cl[j][1])) * wn);
      float v = (gr + gc) / fd[r][c];
      if (i >= g.rows || j >= g.cols) v = 0.f;
      else Gb[(size_t)(g.i0 + i) * max_m + g.j0 + j] = v;
      rsum[r] += v;
      csum[c] += v;
    }
  }
  // row sums: the 16 lanes that share ty, xor tree (fixed order)
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) rsum[r] += __shfl_xor(rsum[r], o, 64);
    const int i = ty + 16 * r;
    if (tx == 0 && i < g.rows) rgpart[(size_t)(g.ra + g.i0 + i) * tiles_m_max + g.j0 / CT] = rsum[r];
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) Cs[ty][tx + 16 * c] = csum[c];
  __syncthreads();
  if (tid < g.cols) {
    float s = 0.f;
    for (int y = 0; y < 16; ++y) s += Cs[y][tid];
    cgpart[(size_t)(g.ca + g.j0 + tid) * tiles_n_max + g.i0 / CT] = s;
  }
}

// dx[row] = (sum over the row's tiles of its G partials, float64, tile order) * x[row]; z = 0 source, 1 target
__global__ __launch_bounds__(64) void k_circle_gfinish(const float* __restrict__ a, const float* __restrict__ bf, int d,
                                                       const int* __restrict__ cu_a, const int* __restrict__ cu_b,
                                                       int tiles_n_max, int tiles_m_max,
                                                       const float* __restrict__ rgpart, const float* __restrict__ cgpart,
                                                       float* __restrict__ da, float* __restrict__ db) {
  const int b = blockIdx.y;
  const bool col = blockIdx.z == 1;
  const int* cu = col ? cu_b : cu_a;
  const int* cv = col ? cu_a : cu_b;
  const int r0 = cu[b], n = cu[b + 1] - r0;
  const int i = blockIdx.x;
  if (i >= n) return;
  const int nt = (cv[b + 1] - cv[b] + CT - 1) / CT, stride = col ? tiles_n_max : tiles_m_max;
  const float* part = (col ? cgpart : rgpart) + (size_t)(r0 + i) * stride;
  double s = 0.0;
  for (int t = 0; t < nt; ++t) s += (double)part[t];
  const float* x = (col ? bf : a) + (size_t)(r0 + i) * d;
  float* y = (col ? db : da) + (size_t)(r0 + i) * d;
  for (int k = threadIdx.x; k < d; k += 64) y[k] = (float)(s * (double)x[k]);
}

struct CircleWs {
  float* axyz;
  float2 *rpart, *cpart;
  unsigned char *rflag, *cflag;
  double2 *rlse, *clse;
  int *rsel, *csel;
  float *rcoef, *ccoef, *rgpart, *cgpart;
};

CircleWs circle_layout(Workspace& w, int nbatch, int max_n, int max_m) {
  const size_t R = (size_t)nbatch * max_n, C = (size_t)nbatch * max_m;
  const size_t tn = cdiv(max_n, CT), tm = cdiv(max_m, CT);
  CircleWs c;
  c.axyz = w.take<float>(R * 3);
  c.rpart = w.take<float2>(R * tm * 2);
  c.cpart = w.take<float2>(C * tn * 2);
  c.rflag = w.take<unsigned char>(R * tm);
  c.cflag = w.take<unsigned char>(C * tn);
  c.rlse = w.take<double2>(R);
  c.clse = w.take<double2>(C);
  c.rsel = w.take<int>(R);
  c.csel = w.take<int>(C);
  c.rcoef = w.take<float>(R);
  c.ccoef = w.take<float>(C);
  c.rgpart = w.take<float>(R * tm);
  c.cgpart = w.take<float>(C * tn);
  return c;
}

// the launches shared by the forward and the backward: transform, tile partials, merged statistics
void circle_stats(const float* a, const float* bf, int d, const float* xa, const float* pose, const float* xb,
                  const int* cu_a, const int* cu_b, int nbatch, int max_n, int max_m, float r_p, float r_n,
                  const CircleWs& c, hipStream_t stream) {
  const int tn = cdiv(max_n, CT), tm = cdiv(max_m, CT);
  hipLaunchKernelGGL(k_circle_transform, dim3(cdiv(max_n, 256), nbatch), dim3(256), 0, stream, pose, xa, cu_a, c.axyz);
  hipLaunchKernelGGL(k_circle_tile, dim3(tn * tm, nbatch), dim3(CB), 0, stream, a, bf, d, c.axyz, xb, cu_a, cu_b, tn,
                     tm, r_p, r_n, c.rpart, c.rflag, c.cpart, c.cflag);
  hipLaunchKernelGGL(k_circle_lse, dim3(cdiv(max_n > max_m ? max_n : max_m, 256), nbatch, 2), dim3(256), 0, stream,
                     cu_a, cu_b, tn, tm, c.rpart, c.rflag, c.cpart, c.cflag, c.rlse, c.rsel, c.clse, c.csel);
}

}  // namespace
}  // namespace spr

using namespace spr;

extern "C" size_t spr_circle_loss_workspace_bytes(int nbatch, int max_n, int max_m) {
  if (nbatch < 1 || max_n < 1 || max_m < 1) return 0;
  return measure(circle_layout, nbatch, max_n, max_m);
}

#define CIRCLE_ARGS_OK                                                                                           \
  (a && bf && xa && pose && xb && cu_a && cu_b && nbatch >= 1 && nbatch <= 65535 && max_n >= 1 && max_m >= 1 && \
   d >= 4 && d % 4 == 0 && ((uintptr_t)a % 16) == 0 && ((uintptr_t)bf % 16) == 0)

extern "C" int spr_circle_loss(const float* a, const float* bf, int d, const float* xa, const float* pose,
                               const float* xb, const int* cu_a, const int* cu_b, int nbatch, int max_n, int max_m,
                               float r_p, float r_n, float* out, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPR_REQUIRE(CIRCLE_ARGS_OK && out, "circle_loss: bad arguments (nbatch=%d max_n=%d max_m=%d d=%d)", nbatch, max_n,
              max_m, d);
  SPR_REQUIRE((long)cdiv(max_n, CT) * cdiv(max_m, CT) < (1l << 31), "circle_loss: grid too large");
  Workspace w(ws, ws_bytes);
  const CircleWs c = circle_layout(w, nbatch, max_n, max_m);
  SPR_REQUIRE(ws != nullptr && w.ok(), "circle_loss: workspace too small");
  circle_stats(a, bf, d, xa, pose, xb, cu_a, cu_b, nbatch, max_n, max_m, r_p, r_n, c, stream);
  hipLaunchKernelGGL(k_circle_pair, dim3(nbatch), dim3(CB), 0, stream, cu_a, cu_b, c.rlse, c.rsel, c.clse, c.csel, out,
                     (const float*)nullptr, (float*)nullptr, (float*)nullptr);
  SPR_LAUNCH_CHECK();
  return 0;
}

extern "C" int spr_circle_loss_bwd(const float* a, const float* bf, int d, const float* xa, const float* pose,
                                   const float* xb, const int* cu_a, const int* cu_b, int nbatch, int max_n,
                                   int max_m, float r_p, float r_n, const float* gout, float* G, float* da, float* db,
                                   void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPR_REQUIRE(CIRCLE_ARGS_OK && gout && G && da && db,
              "circle_loss_bwd: bad arguments (nbatch=%d max_n=%d max_m=%d d=%d)", nbatch, max_n, max_m, d);
  SPR_REQUIRE((long)cdiv(max_n, CT) * cdiv(max_m, CT) < (1l << 31), "circle_loss_bwd: grid too large");
  Workspace w(ws, ws_bytes);
  const CircleWs c = circle_layout(w, nbatch, max_n, max_m);
  SPR_REQUIRE(ws != nullptr && w.ok(), "circle_loss_bwd: workspace too small");
  const int tn = cdiv(max_n, CT), tm = cdiv(max_m, CT);
  circle_stats(a, bf, d, xa, pose, xb, cu_a, cu_b, nbatch, max_n, max_m, r_p, r_n, c, stream);
  hipLaunchKernelGGL(k_circle_pair, dim3(nbatch), dim3(CB), 0, stream, cu_a, cu_b, c.rlse, c.rsel, c.clse, c.csel,
                     (float*)nullptr, gout, c.rcoef, c.ccoef);
  hipLaunchKernelGGL(k_circle_grad, dim3(tn * tm, nbatch), dim3(CB), 0, stream, a, bf, d, c.axyz, xb, cu_a, cu_b, tn,
                     tm, r_p, r_n, c.rlse, c.rcoef, c.clse, c.ccoef, max_n, max_m, G, c.rgpart, c.cgpart);
  hipLaunchKernelGGL(k_circle_gfinish, dim3(max_n > max_m ? max_n : max_m, nbatch, 2), dim3(64), 0, stream, a, bf, d,
                     cu_a, cu_b, tn, tm, c.rgpart, c.cgpart, da, db);
  SPR_LAUNCH_CHECK();
  return 0;
}
