// a11 / a12 / a13 -- dual-softmax matching, Sinkhorn soft correspondences
// and the batched weighted Procrustes (Kabsch) solve on gfx950.
//
// Behaviour contract:
//   RegTR.softmax_correlation   /root/reference/src/models/qk_regtr_full.py:423-672
//     :453 correlation = F_s F_t^T / sqrt(D)
//     :457-459 / :565-567  attn = softmax(dim=-2) * softmax(dim=-1)
//     :468 / :576          val, ind = max over the longer side
//     :525-536 / :635-647  Sinkhorn affinity from the clamped score matrix
//   sinkhorn / compute_rigid_transform_with_sinkhorn  utils/se3_torch.py:166-239
//   compute_rigid_transform                           utils/se3_torch.py:109-163
//
// The reference loops over pairs in Python, materialises softmax copies of the
// N x M matrix and calls LAPACK through torch.svd (plus a device->host sync in
// an assert, se3_torch.py:132).  Here ONE routine, match_head, serves the three
// forward entry points (matches, Sinkhorn correspondences, both): a grouped GEMM
// (spr_linear's arithmetic: range-scaled split-fp16 MFMA by default, exact f32
// in gemm mode 0) writes the scaled score matrices of a group of pairs once into
// scratch (layout: next_pair_off); row / column log-sum-exp sweeps stream them
// (k_row_lse_v: wave per row; k_col_lse_v: 64 columns x 32 row lanes per
// workgroup; with RAW they also reduce the raw matrix in the same read;
// k_row_lse / k_col_lse for the shapes those do not take), the
// Sinkhorn ones through the affinity view (struct Aff) -- the affinity itself is
// stored only by the backward; the
// slack Sinkhorn is carried as two potential vectors
//     u_i = log(1 + sum_j exp(A_ij - v_j)),  v_j = log(1 + sum_i exp(A_ij - u_i))
// (algebraically identical to normalising the zero-padded (N+1)x(M+1) matrix,
// se3_torch.py:186-197), and the pose solve is one workgroup per pair with
// float64 moment accumulation and a 3x3 one-sided Jacobi SVD in registers --
// no host round trip anywhere.
#include <vector>

#include "attn_planes.h"
#include "procrustes_solve.h"
#include "spr_common.h"

namespace spr {
namespace {

struct PairDesc {
  int src_beg, n, tgt_beg, m;
  long long off;  // offset (floats) of this pair's N x M matrix in the scratch
};
// THE layout rule of the scratch: the matrices follow each other, every one starting on a multiple of 64 floats.
// Offset of the matrix after an n x m one at `off`.
__host__ __device__ inline long long next_pair_off(long long off, int n, int m) {
  return (off + (long long)n * m + 63) / 64 * 64;
}

// ---- row / column log-sum-exp over the scaled correlation ------------------
// lse over j of (c[i][j]*scale - sub[j])   (sub may be NULL); optionally +1
// inside the log-sum (the slack entry exp(0)).
// The potentials are float in the forward and double in the backward (PT): the gradients of alpha / beta sum N x M
// terms that cancel down to the slack mass, and an error of 1e-7 in u_i or v_j moves a whole row / column of them
// together -- with float potentials d alpha was off by 4e-4, with double ones by 3e-5 (the terms themselves stay
// float: their rounding errors are independent and average out).
// Optional elementwise view of the stored matrix: the Sinkhorn affinity -(max(x, 0) - softplus(alpha)) / (e^beta +
// 0.02) of the scaled correlation x, evaluated as the passes read it (aff = {scale, softplus alpha, 1 / den} from
// k_epi_params; the same float operations as k_affinity, which the backward uses to store the affinity: bit for bit the
// same values).  The forward never stores the affinity.  aff == nullptr: identity.
struct Aff {
  bool on;
  float sp, inv_den;
  __device__ __forceinline__ explicit Aff(const float* aff)
      : on(aff != nullptr), sp(aff ? aff[1] : 0.f), inv_den(aff ? aff[2] : 0.f) {}
  __device__ __forceinline__ float operator()(float x) const { return on ? -(fmaxf(x, 0.f) - sp) * inv_den : x; }
};
__device__ __forceinline__ float wave_sum_t(float v) { return wave_sum(v); }
__device__ __forceinline__ double wave_sum_t(double v) { return wave_sum_d(v); }
__device__ __forceinline__ float lse_log(float s) { return logf(s); }
__device__ __forceinline__ double lse_log(double s) { return log(s); }

template <typename PT>
__global__ void k_row_lse(const float* __restrict__ mat, const PairDesc* __restrict__ pd,
                          PT* __restrict__ row_out /*packed by src token*/,
                          const PT* __restrict__ col_sub /*packed by tgt token*/, int slack,
                          const float* __restrict__ aff = nullptr) {
  const PairDesc p = pd[blockIdx.y];
  const int row = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (row >= p.n) return;
  const Aff af(aff);
  const float* r = mat + p.off + (size_t)row * p.m;
  float mx = slack ? 0.f : -INFINITY;
  for (int j = lane; j < p.m; j += 64) {
    const float v = (float)((PT)af(r[j]) - (col_sub ? col_sub[p.tgt_beg + j] : (PT)0));
    mx = fmaxf(mx, v);
  }
  mx = wave_max(mx);
  PT s = 0;
  for (int j = lane; j < p.m; j += 64) {
    const PT v = (PT)af(r[j]) - (col_sub ? col_sub[p.tgt_beg + j] : (PT)0);
    s += (PT)expf((float)(v - (PT)mx));
  }
  s = wave_sum_t(s);
  if (slack) s += (PT)expf(0.f - mx);
  if (lane == 0) row_out[p.src_beg + row] = (PT)mx + lse_log(s);
}

// block = 1024 threads: 64 columns x 16 row lanes
constexpr int kColLanes = 16;
template <typename PT>
__global__ __launch_bounds__(1024) void k_col_lse(const float* __restrict__ mat,
                                                 const PairDesc* __restrict__ pd,
                                                 PT* __restrict__ col_out,
                                                 const PT* __restrict__ row_sub, int slack,
                                                 const float* __restrict__ aff = nullptr) {
  const PairDesc p = pd[blockIdx.y];
  const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + cl;
  __shared__ float smx[kColLanes][64];
  __shared__ PT ssum[kColLanes][64];
  const Aff af(aff);
  float mx = -INFINITY;
  PT s = 0;
  if (col < p.m) {
    for (int i = rl; i < p.n; i += kColLanes) {
      const PT vd = (PT)af(mat[p.off + (size_t)i * p.m + col]) - (row_sub ? row_sub[p.src_beg + i] : (PT)0);
      const float v = (float)vd;
      if (v > mx) {
        s = s * (PT)expf(mx - v) + (PT)expf((float)(vd - (PT)v));
        mx = v;
      } else {
        s += (PT)expf((float)(vd - (PT)mx));
      }
    }
  }
  smx[rl][cl] = mx;
  ssum[rl][cl] = s;
  __syncthreads();
  if (rl == 0 && col < p.m) {
    float M = slack ? 0.f : -INFINITY;
    for (int k = 0; k < kColLanes; ++k) M = fmaxf(M, smx[k][cl]);
    PT S = slack ? (PT)expf(0.f - M) : (PT)0;
    for (int k = 0; k < kColLanes; ++k)
      if (smx[k][cl] > -INFINITY) S += ssum[k][cl] * (PT)expf(smx[k][cl] - M);
    col_out[p.tgt_beg + col] = (PT)M + lse_log(S);
  }
}

// e^x through v_exp_f32 with the argument x log2(e) formed in two pieces (the product's rounding error, up to
// 2^-24 |x| log2 e, would otherwise show as a relative error of 4e-6 at |x| = 60): ~1.5 ulp, three instructions
// where expf() spends a dozen on range reduction these passes do not need (x <= 0 here, e^-126 may flush)
__device__ __forceinline__ float exp_neg(float x) {
  x = fmaxf(x, -200.f);                                                       // -inf (masked entries) -> e^-200 = 0
  const float hi = x * 1.44269502162933349609375f;                           // fl32(log2 e)
  const float lo = __builtin_fmaf(x, 1.44269502162933349609375f, -hi);       // product residue (exact)
  return __builtin_amdgcn_exp2f(hi + __builtin_fmaf(x, 1.92596299112661746e-8f, lo));   // + x (log2 e - fl32)
}

typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));

// one wave per row, the whole row (M <= 256 RV) held in registers between the max and the sum.
// RAW: the same read of the row also gives the plain log-sum-exp of the raw matrix (no sub, no view, no slack) in
// raw_out -- the head's first sweep computes the dual softmax's reduction and the first Sinkhorn pass together.  The
// operations of either quantity and their order do not depend on RAW, so neither do the bits.
template <int RV, typename PT, bool RAW>
__global__ __launch_bounds__(256) void k_row_lse_v(const float* __restrict__ mat, const PairDesc* __restrict__ pd,
                                                   PT* __restrict__ row_out, const PT* __restrict__ col_sub,
                                                   int slack, const float* __restrict__ aff,
                                                   PT* __restrict__ raw_out) {
  const PairDesc p = pd[blockIdx.y];
  const int row = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (row >= p.n) return;
  const Aff af(aff);
  const float* r = mat + p.off + (size_t)row * p.m;
  const PT* cs = col_sub ? col_sub + p.tgt_beg : nullptr;
  PT v[RV][4];
  PT vr[RAW ? RV : 1][4];
  float mx = slack ? 0.f : -INFINITY, mxr = -INFINITY;
#pragma unroll
  for (int i = 0; i < RV; ++i) {
    const int j = 4 * (lane + 64 * i);
    if (j + 3 < p.m) {
      typedef PT pt4u __attribute__((ext_vector_type(4), aligned(sizeof(PT))));
      const f4u a = *reinterpret_cast<const f4u*>(r + j);
      pt4u b = {0, 0, 0, 0};
      if (cs) b = *reinterpret_cast<const pt4u*>(cs + j);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if constexpr (RAW) vr[i][e] = a[e] - 0.f;
        v[i][e] = (PT)af(a[e]) - b[e];
      }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if constexpr (RAW) vr[i][e] = j + e < p.m ? r[j + e] - 0.f : -INFINITY;
        v[i][e] = j + e < p.m ? (PT)af(r[j + e]) - (cs ? cs[j + e] : (PT)0) : (PT)-INFINITY;
      }
    }
    if constexpr (RAW)
      mxr = fmaxf(mxr, fmaxf(fmaxf((float)vr[i][0], (float)vr[i][1]), fmaxf((float)vr[i][2], (float)vr[i][3])));
    mx = fmaxf(mx, fmaxf(fmaxf((float)v[i][0], (float)v[i][1]), fmaxf((float)v[i][2], (float)v[i][3])));
  }
  if constexpr (RAW) mxr = wave_max(mxr);
  mx = wave_max(mx);
  PT sr = 0, s = 0;
  if constexpr (RAW) {
#pragma unroll
    for (int i = 0; i < RV; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) sr += (PT)exp_neg((float)(vr[i][e] - (PT)mxr));
  }
#pragma unroll
  for (int i = 0; i < RV; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) s += (PT)exp_neg((float)(v[i][e] - (PT)mx));      // columns past the end: e^-inf = 0
  if constexpr (RAW) sr = wave_sum_t(sr);
  s = wave_sum_t(s);
  if (slack) s += (PT)expf(0.f - mx);
  if (lane == 0) {
    if constexpr (RAW) raw_out[p.src_beg + row] = (PT)mxr + lse_log(sr);
    row_out[p.src_beg + row] = (PT)mx + lse_log(s);
  }
}

// block = 512 threads: 16 column quads (64 columns) x 32 row lanes; four rows in flight per thread, one
// running maximum per column that moves at most once per four rows.  RAW as in k_row_lse_v: quantity 0 is then the
// raw matrix's reduction, the last one (index NQ - 1) the one with sub, slack and view.
constexpr int kColLanesV = 32;
template <typename PT, bool RAW>
__global__ __launch_bounds__(512) void k_col_lse_v(const float* __restrict__ mat, const PairDesc* __restrict__ pd,
                                                  PT* __restrict__ col_out, const PT* __restrict__ row_sub,
                                                  int slack, const float* __restrict__ aff,
                                                  PT* __restrict__ raw_out) {
  constexpr int NQ = RAW ? 2 : 1;
  const PairDesc p = pd[blockIdx.y];
  const Aff af(aff);
  const int cl = threadIdx.x & 15, rl = threadIdx.x >> 4;
  const int col = blockIdx.x * 64 + 4 * cl;
  __shared__ float smx[NQ][kColLanesV][64];
  __shared__ PT ssum[NQ][kColLanesV][64];
  float mx[NQ][4];
  PT s[NQ][4];
#pragma unroll
  for (int w = 0; w < NQ; ++w)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      mx[w][e] = -INFINITY;
      s[w][e] = 0;
    }
  if (col < p.m) {
    // branch-free loads (four rows in flight need their loads back to back): the row index is clamped and masked
    // afterwards; the last, partial column quad reads the row's last four columns and shifts
    const int shift = col + 3 < p.m ? 0 : col - (p.m - 4);          // 0, or 1..3 for the partial quad (M >= 4)
    const float* base = mat + p.off + (col - shift);
    const PT* rs = row_sub ? row_sub + p.src_beg : nullptr;
    for (int i0 = rl; i0 < p.n; i0 += 4 * kColLanesV) {
      f4u a[4];
      PT sub[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = min(i0 + q * kColLanesV, p.n - 1);
        a[q] = *reinterpret_cast<const f4u*>(base + (size_t)i * p.m);
        sub[q] = rs ? rs[i] : (PT)0;
      }
      PT v[NQ][4][4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const bool rok = i0 + q * kColLanesV < p.n;
#pragma unroll
        for (int w = 0; w < NQ; ++w) {
          const bool raw = w + 1 < NQ;
          const float a0 = raw ? a[q][0] : af(a[q][0]), a1 = raw ? a[q][1] : af(a[q][1]),
                      a2 = raw ? a[q][2] : af(a[q][2]), a3 = raw ? a[q][3] : af(a[q][3]);
          const PT sb = raw ? (PT)0 : sub[q];
          const float t0 = shift == 0 ? a0 : shift == 1 ? a1 : shift == 2 ? a2 : a3;
          const float t1 = shift == 0 ? a1 : shift == 1 ? a2 : shift == 2 ? a3 : INFINITY;
          const float t2 = shift == 0 ? a2 : shift == 1 ? a3 : INFINITY;
          const float t3 = shift == 0 ? a3 : INFINITY;
          v[w][q][0] = rok ? (PT)t0 - sb : (PT)-INFINITY;
          v[w][q][1] = rok && t1 < INFINITY ? (PT)t1 - sb : (PT)-INFINITY;
          v[w][q][2] = rok && t2 < INFINITY ? (PT)t2 - sb : (PT)-INFINITY;
          v[w][q][3] = rok && t3 < INFINITY ? (PT)t3 - sb : (PT)-INFINITY;
        }
      }
#pragma unroll
      for (int w = 0; w < NQ; ++w)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float m4 = fmaxf(fmaxf((float)v[w][0][e], (float)v[w][1][e]), fmaxf((float)v[w][2][e], (float)v[w][3][e]));
          if (m4 > mx[w][e]) {
            s[w][e] *= (PT)exp_neg(mx[w][e] - m4);        // first time: 0 * exp(-inf) = 0
            mx[w][e] = m4;
          }
          if (mx[w][e] > -INFINITY) {
            const PT m = (PT)mx[w][e];
            s[w][e] += ((PT)exp_neg((float)(v[w][0][e] - m)) + (PT)exp_neg((float)(v[w][1][e] - m))) +
                       ((PT)exp_neg((float)(v[w][2][e] - m)) + (PT)exp_neg((float)(v[w][3][e] - m)));
          }
        }
    }
  }
#pragma unroll
  for (int w = 0; w < NQ; ++w)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      smx[w][rl][4 * cl + e] = mx[w][e];
      ssum[w][rl][4 * cl + e] = s[w][e];
    }
  __syncthreads();
  if (threadIdx.x < 64 * NQ) {   // wave w finishes quantity w
    const int w = NQ > 1 ? threadIdx.x >> 6 : 0, t = threadIdx.x & 63;
    const int c = blockIdx.x * 64 + t;
    if (c < p.m) {
      const bool sl = w + 1 == NQ && slack;
      float M = sl ? 0.f : -INFINITY;
      for (int k = 0; k < kColLanesV; ++k) M = fmaxf(M, smx[w][k][t]);
      PT S = sl ? (PT)expf(0.f - M) : (PT)0;
      for (int k = 0; k < kColLanesV; ++k)
        if (smx[w][k][t] > -INFINITY) S += ssum[w][k][t] * (PT)expf(smx[w][k][t] - M);
      (w + 1 == NQ ? col_out : raw_out)[p.tgt_beg + c] = (PT)M + lse_log(S);
    }
  }
}

// The only launch sites of the sweeps, for `np` pairs starting at descriptor pg.  raw_out != NULL: the same sweep also
// writes the plain log-sum-exp of the raw matrix there -- float potentials and the shapes of lse_raw_ok only.
inline bool lse_raw_ok(int max_m, int min_m) { return max_m <= 2048 && min_m >= 4; }
template <typename PT>
int launch_row_lse(const float* mat, const PairDesc* pg, int np, int max_n, int max_m, PT* out, const PT* col_sub,
                   int slack, hipStream_t stream, const float* aff = nullptr, PT* raw_out = nullptr) {
  const dim3 grid(cdiv((long)max_n * 64, 256), np);
  auto go = [&](auto kern) {
    hipLaunchKernelGGL(kern, grid, dim3(256), 0, stream, mat, pg, out, col_sub, slack, aff, raw_out);
  };
  if constexpr (sizeof(PT) == 4) {   // (no double instantiation of these: the rows would not fit the register file)
    if (raw_out != nullptr && max_m <= 1024) return go(k_row_lse_v<4, PT, true>), 0;
    if (raw_out != nullptr && max_m <= 2048) return go(k_row_lse_v<8, PT, true>), 0;
    if (raw_out == nullptr && max_m > 2048 && max_m <= 4096) return go(k_row_lse_v<16, PT, false>), 0;
  }
  SPR_REQUIRE(raw_out == nullptr, "row sweep: no two-quantity kernel for this shape or type");
  if (max_m <= 1024)
    go(k_row_lse_v<4, PT, false>);
  else if (max_m <= 2048)
    go(k_row_lse_v<8, PT, false>);
  else
    hipLaunchKernelGGL(k_row_lse<PT>, grid, dim3(256), 0, stream, mat, pg, out, col_sub, slack, aff);
  return 0;
}
template <typename PT>
int launch_col_lse(const float* mat, const PairDesc* pg, int np, int max_m, PT* out, const PT* row_sub, int slack,
                   hipStream_t stream, int min_m, const float* aff = nullptr, PT* raw_out = nullptr) {
  const dim3 grid(cdiv(max_m, 64), np);
  if (raw_out != nullptr) {
    SPR_REQUIRE(sizeof(PT) == 4 && min_m >= 4, "column sweep: no two-quantity kernel for this shape or type");
    if constexpr (sizeof(PT) == 4)
      hipLaunchKernelGGL((k_col_lse_v<PT, true>), grid, dim3(16 * kColLanesV), 0, stream, mat, pg, out, row_sub, slack, aff, raw_out);
  } else if (min_m < 4) {   // (a pair with fewer than four target tokens: the one-column-per-thread form)
    hipLaunchKernelGGL(k_col_lse<PT>, grid, dim3(1024), 0, stream, mat, pg, out, row_sub, slack, aff);
  } else {
    hipLaunchKernelGGL((k_col_lse_v<PT, false>), grid, dim3(16 * kColLanesV), 0, stream, mat, pg, out, row_sub, slack, aff, raw_out);
  }
  return 0;
}

// ---- dual softmax arg-max ---------------------------------------------------
// N > M : for every tgt j   arg max_i  exp(c - col_lse[j]) * exp(c - row_lse[i])
// else  : for every src i   arg max_j  (same product)
__global__ __launch_bounds__(1024) void k_match_cols(const float* __restrict__ mat,
                                                    const PairDesc* __restrict__ pd,
                                                    const float* __restrict__ row_lse,
                                                    const float* __restrict__ col_lse,
                                                    float* __restrict__ val, int* __restrict__ ind,
                                                    float* __restrict__ val2) {
  const PairDesc p = pd[blockIdx.y];
  if (!(p.n > p.m)) return;
  const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + cl;
  __shared__ float sv[kColLanes][64], sv2[kColLanes][64];
  __shared__ int si[kColLanes][64];
  float best = -1.f, second = -1.f;   // second: runner-up value (Lowe ratio test, qk_regtr_full.py:370-384)
  int bi = 0;
  if (col < p.m) {
    const float cl_j = col_lse[p.tgt_beg + col];
    for (int i = rl; i < p.n; i += kColLanes) {
      const float c = mat[p.off + (size_t)i * p.m + col];
      const float a = expf(c - cl_j) * expf(c - row_lse[p.src_beg + i]);
      if (a > best) {
        second = best;
        best = a;
        bi = i;
      } else if (a > second) {
        second = a;
      }
    }
  }
  sv[rl][cl] = best;
  sv2[rl][cl] = second;
  si[rl][cl] = bi;
  __syncthreads();
  if (rl == 0 && col < p.m) {
    for (int k = 1; k < kColLanes; ++k) {
      const float b = sv[k][cl], b2 = sv2[k][cl];
      const int i = si[k][cl];
      if (b > best || (b == best && i < bi)) {
        second = fmaxf(best, b2);
        best = b;
        bi = i;
      } else {
        second = fmaxf(second, b);
      }
    }
    val[p.tgt_beg + col] = best;
    ind[p.tgt_beg + col] = bi;
    if (val2) val2[p.tgt_beg + col] = second;
  }
}

__global__ void k_match_rows(const float* __restrict__ mat, const PairDesc* __restrict__ pd,
                             const float* __restrict__ row_lse, const float* __restrict__ col_lse,
                             float* __restrict__ val, int* __restrict__ ind, float* __restrict__ val2) {
  const PairDesc p = pd[blockIdx.y];
  if (p.n > p.m) return;
  const int row = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (row >= p.n) return;
  const float rl_i = row_lse[p.src_beg + row];
  float best = -1.f, second = -1.f;
  int bj = 0;
  for (int j = lane; j < p.m; j += 64) {
    const float c = mat[p.off + (size_t)row * p.m + j];
    const float a = expf(c - col_lse[p.tgt_beg + j]) * expf(c - rl_i);
    if (a > best) {
      second = best;
      best = a;
      bj = j;
    } else if (a > second) {
      second = a;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float b = __shfl_xor(best, o, 64), b2 = __shfl_xor(second, o, 64);
    const int j = __shfl_xor(bj, o, 64);
    if (b > best || (b == best && j < bj)) {
      second = fmaxf(best, b2);
      best = b;
      bj = j;
    } else {
      second = fmaxf(second, b);
    }
  }
  if (lane == 0) {
    val[p.src_beg + row] = best;
    ind[p.src_beg + row] = bj;
    if (val2) val2[p.src_beg + row] = second;
  }
}

// ---- residuals of pose hypotheses (LGR re-weighting, RANSAC scoring; qk_regtr_full.py:386-421) ----
// res[i] = || b_i - (R_s a_i + t_s) ||  for the points of set s (pair_cu), one pose per set
__global__ void k_pose_residuals(const float* __restrict__ pose, const float* __restrict__ a,
                                 const float* __restrict__ b, const int* __restrict__ pair_cu, int npairs,
                                 float* __restrict__ res) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int total = pair_cu[npairs];
  if (i >= total) return;
  const int s = find_segment(pair_cu, npairs, i);
  const float* T = pose + 12 * (size_t)s;
  const float x = a[3 * (size_t)i], y = a[3 * (size_t)i + 1], z = a[3 * (size_t)i + 2];
  float d2 = 0.f;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const float v = b[3 * (size_t)i + r] - ((x * T[4 * r] + y * T[4 * r + 1] + z * T[4 * r + 2]) + T[4 * r + 3]);
    d2 += v * v;
  }
  res[i] = sqrtf(d2);
}
// score[h] = mean_i || b_i - T_h a_i ||  over ONE point set for H hypotheses (one wave per hypothesis)
__global__ void k_pose_scores(const float* __restrict__ poses, int nh, const float* __restrict__ a,
                              const float* __restrict__ b, int n, float* __restrict__ score) {
  const int h = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  if (h >= nh) return;
  const float* T = poses + 12 * (size_t)h;
  float s = 0.f;
  for (int i = lane; i < n; i += 64) {
    const float x = a[3 * (size_t)i], y = a[3 * (size_t)i + 1], z = a[3 * (size_t)i + 2];
    float d2 = 0.f;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const float v = b[3 * (size_t)i + r] - ((x * T[4 * r] + y * T[4 * r + 1] + z * T[4 * r + 2]) + T[4 * r + 3]);
      d2 += v * v;
    }
    s += sqrtf(d2);
  }
  s = wave_sum(s);
  if (lane == 0) score[h] = s / (float)n;
}

// ---- elementwise transforms of the score matrix -----------------------------
__global__ void k_scale(float* __restrict__ mat, long long total, float s) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < total) mat[i] *= s;
}
// affinity = -(max(c*scale, 0) - sp_alpha) * inv_den      (qk_regtr_full.py:532-535)
// alpha, beta: the model's learnable scalars, read from DEVICE memory (no host round trip);
// softplus with threshold 20 like torch.nn.Softplus, evaluated in float64.
// parameters of the epilogues and of the affinity view: [0] = scale, [1] = softplus(alpha),
// [2] = 1 / (exp(beta) + 0.02)
__global__ void k_epi_params(float scale, const float* __restrict__ alpha_p, const float* __restrict__ beta_p,
                             float* __restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  out[0] = scale;
  if (alpha_p != nullptr) {
    const float alpha = alpha_p[0], beta = beta_p[0];
    out[1] = (float)(alpha > 20.f ? (double)alpha : log1p(exp((double)alpha)));
    out[2] = (float)(1.0 / (exp((double)beta) + 0.02));
  }
}

// in place, epi = {scale, softplus alpha, 1 / den} from k_epi_params
__global__ void k_affinity(float* __restrict__ mat, long long total, const float* __restrict__ epi) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < total) {
    const float sc = fmaxf(mat[i] * epi[0], 0.f);
    mat[i] = -(sc - epi[1]) * epi[2];
  }
}

// w_i = sum_j P_ij ; t_hat_i = sum_j P_ij tgt_j / (w_i + 1e-6),  P = exp(A - u_i - v_j)
__global__ void k_sinkhorn_final(const float* __restrict__ mat, const PairDesc* __restrict__ pd,
                                 const float* __restrict__ u, const float* __restrict__ v,
                                 const float* __restrict__ xyz, float* __restrict__ out_w,
                                 float* __restrict__ out_t, const float* __restrict__ aff = nullptr) {
  const PairDesc p = pd[blockIdx.y];
  const int row = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (row >= p.n) return;
  const Aff af(aff);
  const float ui = u[p.src_beg + row];
  float w = 0.f, tx = 0.f, ty = 0.f, tz = 0.f;
  for (int j = lane; j < p.m; j += 64) {
    const float pij = expf(af(mat[p.off + (size_t)row * p.m + j]) - ui - v[p.tgt_beg + j]);
    const float* t = xyz + 3 * (size_t)(p.tgt_beg + j);
    w += pij;
    tx += pij * t[0];
    ty += pij * t[1];
    tz += pij * t[2];
  }
  w = wave_sum(w);
  tx = wave_sum(tx);
  ty = wave_sum(ty);
  tz = wave_sum(tz);
  if (lane == 0) {
    // packed by src token; src tokens of pair b start at src_beg (global)
    const float d = w + 1e-6f;
    out_w[p.src_beg + row] = w;
    out_t[3 * (size_t)(p.src_beg + row) + 0] = tx / d;
    out_t[3 * (size_t)(p.src_beg + row) + 1] = ty / d;
    out_t[3 * (size_t)(p.src_beg + row) + 2] = tz / d;
  }
}

// ---- weighted Procrustes: the solve is procrustes_solve.h (shared with refine.hip) ------------
__global__ __launch_bounds__(256) void k_procrustes(const float* __restrict__ a,
                                                    const float* __restrict__ b,
                                                    const float* __restrict__ w,
                                                    const int* __restrict__ pair_cu,
                                                    float* __restrict__ out) {
  const int pr = blockIdx.x;
  const int beg = pair_cu[pr], end = pair_cu[pr + 1];
  __shared__ double sh[256];
  const float* pa = a + 3 * (size_t)beg;
  const float* pb = b + 3 * (size_t)beg;
  const float* pw = w ? w + beg : nullptr;
  procrustes_block(
      end - beg, w != nullptr, [&](int i, int d) { return pa[3 * (size_t)i + d]; },
      [&](int i, int d) { return pb[3 * (size_t)i + d]; }, [&](int i) { return pw[i]; }, sh,
      out + 12 * (size_t)pr);
}

// ---- weighted Procrustes backward (se3_torch.py:109-163 differentiated; the reference relies on
// torch.svd's autograd) -------------------------------------------------------------------------
// With H = sum w~ (a - abar)(b - bbar)^T = U S V^T and R = V D U^T:  H^T = R P,  P = U L U^T,
// L = diag(s1, s2, d s3).  For a perturbation dH:  R^T dR = Om (skew) solves
// Om P + P Om = Z - Z^T, Z = R^T dH^T, i.e. in P's eigenbasis Om~_ij = (Z - Z^T)~_ij / (l_i + l_j).
// Adjoint: with Y = R^T G_R, Q = U [ (U^T (Y - Y^T)/2 U)_ij / (l_i + l_j) ] U^T,
//   dL/dH = -2 Q R^T.
// Then dL/db_i = w~_i (dL/dH^T (a_i - abar) + g_t), dL/dw~_i = (a_i - abar)^T dL/dH (b_i - bbar)
// - (R^T g_t) . a_i + g_t . b_i, and w~ = w / sum(w).
__global__ __launch_bounds__(256) void k_procrustes_bwd(const float* __restrict__ a, const float* __restrict__ b,
                                                        const float* __restrict__ w,
                                                        const int* __restrict__ pair_cu,
                                                        const float* __restrict__ dpose, float* __restrict__ da,
                                                        float* __restrict__ db, float* __restrict__ dw) {
  const int pr = blockIdx.x;
  const int beg = pair_cu[pr], end = pair_cu[pr + 1];
  __shared__ double sh[256];
  __shared__ double bc[32];   // GH (9), g_t (3), g_abar (3)
  double acc[7] = {0, 0, 0, 0, 0, 0, 0};
  for (int i = beg + threadIdx.x; i < end; i += 256) {
    const double wi = w ? (double)w[i] : 1.0;
    acc[0] += wi;
    for (int d = 0; d < 3; ++d) {
      acc[1 + d] += wi * (double)a[3 * (size_t)i + d];
      acc[4 + d] += wi * (double)b[3 * (size_t)i + d];
    }
  }
  block_reduce_d(acc, 7, sh);
  const bool clamped = w ? acc[0] < 1e-6 : acc[0] < 1.0;
  const double den = w ? fmax(acc[0], 1e-6) : fmax(acc[0], 1.0);
  double ca[3], cb[3];
  for (int d = 0; d < 3; ++d) {
    ca[d] = acc[1 + d] / den;
    cb[d] = acc[4 + d] / den;
  }
  double cov[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = beg + threadIdx.x; i < end; i += 256) {
    const double wi = (w ? (double)w[i] : 1.0) / den;
    double da_[3], db_[3];
    for (int d = 0; d < 3; ++d) {
      da_[d] = (double)a[3 * (size_t)i + d] - ca[d];
      db_[d] = ((double)b[3 * (size_t)i + d] - cb[d]) * wi;
    }
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) cov[3 * r + c] += da_[r] * db_[c];
  }
  block_reduce_d(cov, 9, sh);
  if (threadIdx.x == 0) {
    double A[3][3], U[3][3], S[3], V[3][3], R[3][3];
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) A[r][c] = cov[3 * r + c];
    svd3_jacobi(A, U, S, V);
    double dsign = 1.0;
    for (int pass = 0; pass < 2; ++pass) {
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) R[r][c] = V[r][0] * U[c][0] + V[r][1] * U[c][1] + V[r][2] * U[c][2];
      const double det = R[0][0] * (R[1][1] * R[2][2] - R[1][2] * R[2][1]) -
                         R[0][1] * (R[1][0] * R[2][2] - R[1][2] * R[2][0]) +
                         R[0][2] * (R[1][0] * R[2][1] - R[1][1] * R[2][0]);
      if (det > 0.0) break;
      for (int r = 0; r < 3; ++r) V[r][2] = -V[r][2];
      dsign = -1.0;
    }
    const float* G = dpose + 12 * (size_t)pr;
    double GR[3][3], gt[3];
    for (int r = 0; r < 3; ++r) {
      gt[r] = (double)G[4 * r + 3];
      for (int c = 0; c < 3; ++c) GR[r][c] = (double)G[4 * r + c] - gt[r] * ca[c];   // t = bbar - R abar
    }
    const double lam[3] = {S[0], S[1], dsign * S[2]};
    double Y[3][3], Ysk[3][3], T1[3][3], Yt[3][3], Qt[3][3], Q[3][3], GH[3][3];
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) Y[r][c] = R[0][r] * GR[0][c] + R[1][r] * GR[1][c] + R[2][r] * GR[2][c];
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) Ysk[r][c] = 0.5 * (Y[r][c] - Y[c][r]);
    for (int r = 0; r < 3; ++r)      // T1 = U^T Ysk
      for (int c = 0; c < 3; ++c) T1[r][c] = U[0][r] * Ysk[0][c] + U[1][r] * Ysk[1][c] + U[2][r] * Ysk[2][c];
    for (int r = 0; r < 3; ++r)      // Yt = T1 U
      for (int c = 0; c < 3; ++c) Yt[r][c] = T1[r][0] * U[0][c] + T1[r][1] * U[1][c] + T1[r][2] * U[2][c];
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) {
        const double s = lam[r] + lam[c];
        Qt[r][c] = (r != c && fabs(s) > 1e-300) ? Yt[r][c] / s : 0.0;
      }
    for (int r = 0; r < 3; ++r)      // T1 = U Qt
      for (int c = 0; c < 3; ++c) T1[r][c] = U[r][0] * Qt[0][c] + U[r][1] * Qt[1][c] + U[r][2] * Qt[2][c];
    for (int r = 0; r < 3; ++r)      // Q = T1 U^T
      for (int c = 0; c < 3; ++c) Q[r][c] = T1[r][0] * U[c][0] + T1[r][1] * U[c][1] + T1[r][2] * U[c][2];
    for (int r = 0; r < 3; ++r)      // GH = -2 Q R^T
      for (int c = 0; c < 3; ++c) GH[r][c] = -2.0 * (Q[r][0] * R[c][0] + Q[r][1] * R[c][1] + Q[r][2] * R[c][2]);
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) bc[3 * r + c] = GH[r][c];
      bc[9 + r] = gt[r];
      bc[12 + r] = -(R[0][r] * gt[0] + R[1][r] * gt[1] + R[2][r] * gt[2]);   // g_abar = -R^T g_t
    }
  }
  __syncthreads();
  double GH[9], gt[3], ga[3];
  for (int k = 0; k < 9; ++k) GH[k] = bc[k];
  for (int k = 0; k < 3; ++k) {
    gt[k] = bc[9 + k];
    ga[k] = bc[12 + k];
  }
  // Below the clamp the normalised weights sum to s = sum w / 1e-6 < 1, and H = sum w~ a b^T - (2 - s) abar bbar^T
  // keeps a dependence on the centroids that vanishes at s = 1: om = 1 - s, GHcb = GH bbar, GHca = GH^T abar.
  const double om = clamped ? 1.0 - acc[0] / den : 0.0;
  double GHcb[3], GHca[3];
  for (int r = 0; r < 3; ++r) {
    GHcb[r] = om * (GH[3 * r] * cb[0] + GH[3 * r + 1] * cb[1] + GH[3 * r + 2] * cb[2]);
    GHca[r] = om * (GH[r] * ca[0] + GH[3 + r] * ca[1] + GH[6 + r] * ca[2]);
  }
  // first pass: dL/dw~_i and its weighted sum
  double s2[1] = {0.0};
  for (int i = beg + threadIdx.x; i < end; i += 256) {
    const double wt = (w ? (double)w[i] : 1.0) / den;
    double ac[3], bcv[3], ai[3], bi[3];
    for (int d = 0; d < 3; ++d) {
      ai[d] = (double)a[3 * (size_t)i + d];
      bi[d] = (double)b[3 * (size_t)i + d];
      ac[d] = ai[d] - ca[d];
      bcv[d] = bi[d] - cb[d];
    }
    double q = 0.0;
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) q += ac[r] * GH[3 * r + c] * bcv[c];
    for (int d = 0; d < 3; ++d) q += ga[d] * ai[d] + gt[d] * bi[d];
    if (clamped) q -= ai[0] * GHcb[0] + ai[1] * GHcb[1] + ai[2] * GHcb[2] + GHca[0] * bi[0] + GHca[1] * bi[1] + GHca[2] * bi[2];
    s2[0] += wt * q;
    if (db)
      for (int c = 0; c < 3; ++c)
        db[3 * (size_t)i + c] =
            (float)(wt * (GH[c] * ac[0] + GH[3 + c] * ac[1] + GH[6 + c] * ac[2] + gt[c] - (clamped ? GHca[c] : 0.0)));
    if (da)
      for (int r = 0; r < 3; ++r)
        da[3 * (size_t)i + r] = (float)(wt * (GH[3 * r] * bcv[0] + GH[3 * r + 1] * bcv[1] + GH[3 * r + 2] * bcv[2] +
                                              ga[r] - (clamped ? GHcb[r] : 0.0)));
    if (dw) dw[i] = (float)q;   // completed below
  }
  block_reduce_d(s2, 1, sh);
  if (dw) {
    __syncthreads();
    for (int i = beg + threadIdx.x; i < end; i += 256)
      dw[i] = (float)(((double)dw[i] - (clamped ? 0.0 : s2[0])) / den);
  }
}

// ---- Sinkhorn (slack) backward -------------------------------------------------------------------
// Forward (spr_sinkhorn_correspondences): v_0 = 0; for t = 1..n: u_t = log(1 + sum_j e^{A_ij - v_{t-1,j}}),
// v_t = log(1 + sum_i e^{A_ij - u_{t,i}});  P = e^{A - u_n - v_n};  w_i = sum_j P_ij,
// that_i = sum_j P_ij tgt_j / (w_i + 1e-6).
// Final step, row part: Y_ij = gP_ij P_ij with gP_ij = dw_i + dthat_i . (tgt_j - that_i) / (w_i + 1e-6);
// dA = Y, du_i = -sum_j Y_ij.   One wave per src row.
__global__ void k_sk_bwd_final(const float* __restrict__ mat, float* __restrict__ dmat,
                               const PairDesc* __restrict__ pd, const double* __restrict__ u,
                               const double* __restrict__ v, const float* __restrict__ xyz,
                               const float* __restrict__ dw, const float* __restrict__ dthat,
                               float* __restrict__ du) {
  const PairDesc p = pd[blockIdx.y];
  const int row = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  if (row >= p.n) return;
  const int gi = p.src_beg + row;
  const double ui = u[gi];
  const float* ar = mat + p.off + (size_t)row * p.m;
  float* dr = dmat + p.off + (size_t)row * p.m;
  float wsum = 0.f, tx = 0.f, ty = 0.f, tz = 0.f;
  for (int j = lane; j < p.m; j += 64) {
    const float pij = expf((float)((double)ar[j] - ui - v[p.tgt_beg + j]));
    const float* t = xyz + 3 * (size_t)(p.tgt_beg + j);
    wsum += pij;
    tx += pij * t[0];
    ty += pij * t[1];
    tz += pij * t[2];
  }
  wsum = wave_sum(wsum);
  tx = wave_sum(tx);
  ty = wave_sum(ty);
  tz = wave_sum(tz);
  const float dn = wsum + 1e-6f;
  const float hx = tx / dn, hy = ty / dn, hz = tz / dn;
  const float gw = dw[gi], gx = dthat[3 * (size_t)gi], gy = dthat[3 * (size_t)gi + 1], gz = dthat[3 * (size_t)gi + 2];
  float s = 0.f;
  for (int j = lane; j < p.m; j += 64) {
    const float pij = expf((float)((double)ar[j] - ui - v[p.tgt_beg + j]));
    const float* t = xyz + 3 * (size_t)(p.tgt_beg + j);
    const float gp = gw + (gx * (t[0] - hx) + gy * (t[1] - hy) + gz * (t[2] - hz)) / dn;
    const float y = gp * pij;
    dr[j] = y;
    s += y;
  }
  s = wave_sum(s);
  if (lane == 0) du[gi] = -s;
}
// column sums of dmat: dv_j = -sum_i dmat_ij  (64 columns x 16 row lanes)
__global__ __launch_bounds__(1024) void k_sk_colsum_neg(const float* __restrict__ dmat,
                                                       const PairDesc* __restrict__ pd, float* __restrict__ dv) {
  const PairDesc p = pd[blockIdx.y];
  const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + cl;
  __shared__ float ss[kColLanes][64];
  float s = 0.f;
  if (col < p.m)
    for (int i = rl; i < p.n; i += kColLanes) s += dmat[p.off + (size_t)i * p.m + col];
  ss[rl][cl] = s;
  __syncthreads();
  if (rl == 0 && col < p.m) {
    float t = 0.f;
    for (int k = 0; k < kColLanes; ++k) t += ss[k][cl];
    dv[p.tgt_beg + col] = -t;
  }
}
// column step of iteration t (v_t from u_t): C_ij = e^{A_ij - u_i - v_j}; dA_ij += dv_j C_ij;
// du_i -= sum_j dv_j C_ij.   One wave per src row.
__global__ void k_sk_bwd_col(const float* __restrict__ mat, float* __restrict__ dmat,
                             const PairDesc* __restrict__ pd, const double* __restrict__ u,
                             const double* __restrict__ v, const float* __restrict__ dv, float* __restrict__ du) {
  const PairDesc p = pd[blockIdx.y];
  const int row = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  if (row >= p.n) return;
  const int gi = p.src_beg + row;
  const double ui = u[gi];
  const float* ar = mat + p.off + (size_t)row * p.m;
  float* dr = dmat + p.off + (size_t)row * p.m;
  float s = 0.f;
  for (int j = lane; j < p.m; j += 64) {
    const float c = dv[p.tgt_beg + j] * expf((float)((double)ar[j] - ui - v[p.tgt_beg + j]));
    dr[j] += c;
    s += c;
  }
  s = wave_sum(s);
  if (lane == 0) du[gi] -= s;
}
// row step of iteration t (u_t from v_{t-1}): R_ij = e^{A_ij - v_j - u_i}; dA_ij += du_i R_ij;
// dv_prev_j = -sum_i du_i R_ij  (written, not accumulated: v_{t-1} has no other consumer).
__global__ __launch_bounds__(1024) void k_sk_bwd_row(const float* __restrict__ mat, float* __restrict__ dmat,
                                                    const PairDesc* __restrict__ pd, const double* __restrict__ u,
                                                    const double* __restrict__ vprev,
                                                    const float* __restrict__ du, float* __restrict__ dvprev) {
  const PairDesc p = pd[blockIdx.y];
  const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + cl;
  __shared__ float ss[kColLanes][64];
  float s = 0.f;
  if (col < p.m) {
    const double vj = vprev ? vprev[p.tgt_beg + col] : 0.0;
    for (int i = rl; i < p.n; i += kColLanes) {
      const size_t o = p.off + (size_t)i * p.m + col;
      const float r = du[p.src_beg + i] * expf((float)((double)mat[o] - vj - u[p.src_beg + i]));
      dmat[o] += r;
      s += r;
    }
  }
  ss[rl][cl] = s;
  __syncthreads();
  if (dvprev && rl == 0 && col < p.m) {
    float t = 0.f;
    for (int k = 0; k < kColLanes; ++k) t += ss[k][cl];
    dvprev[p.tgt_beg + col] = -t;
  }
}
// affinity backward: A = -(max(c s, 0) - sp) inv_den.  In place: dmat <- d corr = -dA inv_den s [c s > 0];
// per-block partial sums of dA and dA * A (for d alpha, d beta) in float64.
__global__ __launch_bounds__(256) void k_affinity_bwd(const float* __restrict__ corr, const float* __restrict__ amat,
                                                      float* __restrict__ dmat, long long total, float scale,
                                                      const float* __restrict__ beta_p, double* __restrict__ parts) {
  __shared__ double sh[4];
  const float inv_den = (float)(1.0 / (exp((double)beta_p[0]) + 0.02));
  double s1 = 0.0, s2 = 0.0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const float dA = dmat[i];   // alignment padding between pairs holds zeros (memset by the caller)
    s1 += (double)dA;
    if (dA != 0.f) s2 += (double)dA * (double)amat[i];
    dmat[i] = corr[i] * scale > 0.f ? -dA * inv_den * scale : 0.f;
  }
  s1 = block_sum_d(s1, sh);
  s2 = block_sum_d(s2, sh);
  if (threadIdx.x == 0) {
    parts[2 * blockIdx.x] = s1;
    parts[2 * blockIdx.x + 1] = s2;
  }
}
// d alpha = (sum dA) inv_den sigmoid(alpha);  d beta = (sum dA A) (-e^beta / den)
__global__ void k_affinity_bwd_final(const double* __restrict__ parts, int nparts, const float* __restrict__ alpha_p,
                                     const float* __restrict__ beta_p, float* __restrict__ dalpha,
                                     float* __restrict__ dbeta) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double s1 = 0.0, s2 = 0.0;
  for (int i = 0; i < nparts; ++i) {
    s1 += parts[2 * i];
    s2 += parts[2 * i + 1];
  }
  const double al = (double)alpha_p[0], be = (double)beta_p[0];
  const double den = exp(be) + 0.02;
  const double sig = al > 20.0 ? 1.0 : 1.0 / (1.0 + exp(-al));
  dalpha[0] = (float)(s1 / den * sig);
  dbeta[0] = (float)(-s2 * exp(be) / den);
}
// device descriptors for the two feature-gradient GEMMs (spr_bgemm records)
struct GemmRec {
  long long a_off, b_off, c_off;
  int m, n, k, pad;
};
__global__ void k_build_grad_recs(const PairDesc* __restrict__ pd, int npairs, int d, GemmRec* rs, GemmRec* rt) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= npairs) return;
  const PairDesc p = pd[b];
  // dFs[n, d] = dcorr[n, m] Ft[m, d]
  rs[b] = GemmRec{p.off, (long long)p.tgt_beg * d, (long long)p.src_beg * d, p.n, d, p.m, p.m};   // pad = lda
  // dFt[m, d] = dcorr^T[m, n] Fs[n, d]
  rt[b] = GemmRec{p.off, (long long)p.src_beg * d, (long long)p.tgt_beg * d, p.m, d, p.n, p.m};
}

// descriptors of all pairs on the host; returns the scratch's size in floats
long long build_pairs(const int* cu_host, int npairs, PairDesc* h) {
  long long off = 0;
  for (int b = 0; b < npairs; ++b) {
    h[b] = PairDesc{cu_host[b], cu_host[b + 1] - cu_host[b], cu_host[npairs + b],
                    cu_host[npairs + b + 1] - cu_host[npairs + b], off};
    off = next_pair_off(off, h[b].n, h[b].m);
  }
  return off;
}

// The correlation scratch and everything corr_setup needs around it.  split: gemm_mode() == 1, the grouped split-fp16
// product with its tile records and the two operand ranges (the size queries measure with them).
struct CorrWs {
  size_t total;   // floats of mat
  float* mat;
  PairDesc* pd;
  GemmGroup* gg;
  float *sparts, *tparts;
};
CorrWs corr_layout(Workspace& w, const int* cu_host, int npairs, bool split) {
  long long off = 0;
  for (int b = 0; b < npairs; ++b)
    off = next_pair_off(off, cu_host[b + 1] - cu_host[b], cu_host[npairs + b + 1] - cu_host[npairs + b]);
  CorrWs l{};
  l.total = (size_t)off;
  l.mat = w.take<float>(l.total);
  l.pd = w.take<PairDesc>(npairs);
  if (split) {
    l.gg = w.take<GemmGroup>(npairs);
    l.sparts = w.take<float>(kAmaxParts);
    l.tparts = w.take<float>(kAmaxParts);
  }
  return l;
}
// The matching head (spr_match_workspace_bytes = spr_sinkhorn_workspace_bytes measure it with both heads wanted).
struct HeadWs {
  float* epi;   // {scale, softplus alpha, 1 / (e^beta + 0.02)}: the epilogue reads [0], the view all
  CorrWs corr;
  float *row_lse, *col_lse, *u, *v;
};
HeadWs head_layout(Workspace& w, const int* cu_host, int npairs, bool split, bool want_match, bool want_sinkhorn) {
  const size_t T = (size_t)cu_host[2 * npairs];
  HeadWs l{};
  l.epi = w.take<float>(4);
  l.corr = corr_layout(w, cu_host, npairs, split);
  if (want_match) {
    l.row_lse = w.take<float>(T);
    l.col_lse = w.take<float>(T);
  }
  if (want_sinkhorn) {
    l.u = w.take<float>(T);
    l.v = w.take<float>(T);
  }
  (void)w.take<char>(1792);   // unused: the size query has always counted it, and callers see the same size as before
  return l;
}
// spr_sinkhorn_bwd
struct SinkhornBwdWs {
  CorrWs corr;
  float *corr_copy, *dmat;
  GemmRec *rs, *rt;
  double *U, *V;   // [max(n_iters, 1)][T] potentials in double (see k_row_lse)
  float *du, *dva, *dvb;
  double *zero, *parts;
  float* epi;
};
SinkhornBwdWs sinkhorn_bwd_layout(Workspace& w, const int* cu_host, int npairs, int n_iters, bool split) {
  const size_t T = (size_t)cu_host[2 * npairs], it = (size_t)(n_iters > 0 ? n_iters : 1);
  SinkhornBwdWs l;
  l.corr = corr_layout(w, cu_host, npairs, split);
  l.corr_copy = w.take<float>(l.corr.total);
  l.dmat = w.take<float>(l.corr.total);
  l.rs = w.take<GemmRec>(npairs);
  l.rt = w.take<GemmRec>(npairs);
  l.U = w.take<double>(it * T);
  l.V = w.take<double>(it * T);
  l.du = w.take<float>(T);
  l.dva = w.take<float>(T);
  l.dvb = w.take<float>(T);
  l.zero = w.take<double>(T);
  l.parts = w.take<double>(2 * 1024);
  l.epi = w.take<float>(4);
  // unused: the size query has always counted U, V and zero as 4 it + 2 float arrays of T, each rounded up on its own,
  // and 2816 bytes more; callers see the same size as before
  const size_t a4 = align_up(T * 4, 256);
  (void)w.take<char>((4 * it + 2) * a4 - 2 * align_up(it * T * 8, 256) - align_up(T * 8, 256) + 2816);
  return l;
}

}  // namespace
}  // namespace spr

using namespace spr;

extern "C" size_t spr_match_workspace_bytes(const int* cu_host, int npairs) {
  return measure(head_layout, cu_host, npairs, true, true, true);
}
extern "C" size_t spr_sinkhorn_workspace_bytes(const int* cu_host, int npairs) {
  return spr_match_workspace_bytes(cu_host, npairs);
}

namespace {
// Fills the scratch with raw correlations F_s F_t^T (unscaled), one MFMA GEMM
// per pair; uploads the pair descriptors.
// per_group: the running tile count restarts every per_group pairs (the correlation GEMM is launched once per
// group of pairs, see correlate)
__global__ void k_build_pairs(const int* __restrict__ cu, int npairs, PairDesc* pd, GemmGroup* gg, int d,
                              int bm, int bn, int per_group) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  long long off = 0;
  int tiles = 0;
  for (int b = 0; b < npairs; ++b) {
    if (b % per_group == 0) tiles = 0;
    PairDesc p;
    p.src_beg = cu[b];
    p.n = cu[b + 1] - cu[b];
    p.tgt_beg = cu[npairs + b];
    p.m = cu[npairs + b + 1] - cu[npairs + b];
    p.off = off;
    if (gg != nullptr) {   // the pair's correlation GEMM as one group of the grouped launch
      GemmGroup g;
      g.a_off = (long long)p.src_beg * d;
      g.b_off = (long long)p.tgt_beg * d;
      g.c_off = off;
      g.m = p.n;
      g.n = p.m;
      tiles += ((p.n + bm - 1) / bm) * ((p.m + bn - 1) / bn);
      g.tile_end = tiles;
      g.pad = 0;
      gg[b] = g;
    }
    off = next_pair_off(off, p.n, p.m);
    pd[b] = p;
  }
}

// Correlation matrices of all pairs, produced and consumed GROUP BY GROUP: the score matrices of the bench's 32
// pairs are 477 MB and every softmax / Sinkhorn pass swept all of them from HBM (nine to thirteen sweeps per
// forward); the matrices of a group are written by their GEMM and read by all their passes while (mostly) still in
// the 256 MB Infinity Cache.  Group budget 250 MB = 16 of the bench's pairs (measured: 96 MB groups leave the chip
// under-filled -- 3.9 ms of matching kernels per forward; 250 MB: 2.6 ms; one group of 477 MB: 3.0 ms).  corr_setup builds the descriptors of all pairs, corr_gemm launches the
// product of one group.
// epi_mode / epi: optional elementwise epilogue of the grouped GEMM (kEpiScale; parameters on the
// device); applied = whether it ran (split-fp16 mode) or the separate pass over the matrix is still needed
// (exact-f32 mode: one GEMM per pair).
struct Corr {
  const float* feat;
  int d, npairs;
  float* mat;
  PairDesc* pd;
  GemmGroup* gg;
  std::vector<PairDesc> h;
  long long total;
  int max_n, max_m, min_m, per_group, ngroups;
  bool grouped;
  const float *sparts, *tparts;
  int first(int g) const { return g * per_group; }
  int count(int g) const { return (g + 1) * per_group <= npairs ? per_group : npairs - g * per_group; }
  // element range of group g inside mat
  long long beg(int g) const { return h[first(g)].off; }
  long long end(int g) const {
    const int l = first(g) + count(g) - 1;
    return l + 1 < npairs ? h[l + 1].off : total;
  }
};
int corr_setup(Corr& c, const float* feat, int d, const int* cu_dev, const int* cu_host, int npairs, const CorrWs& cw,
               bool split, hipStream_t stream, bool one_group) {
  c.feat = feat;
  c.d = d;
  c.npairs = npairs;
  c.h.resize(npairs);
  c.total = build_pairs(cu_host, npairs, c.h.data());
  c.mat = cw.mat;
  c.pd = cw.pd;
  c.max_n = 0;
  c.max_m = 0;
  c.min_m = 1 << 30;
  for (int b = 0; b < npairs; ++b) {
    SPR_REQUIRE(c.h[b].n > 0 && c.h[b].m > 0, "match: empty cloud in pair %d", b);
    c.max_n = c.h[b].n > c.max_n ? c.h[b].n : c.max_n;
    c.max_m = c.h[b].m > c.max_m ? c.h[b].m : c.max_m;
    c.min_m = c.h[b].m < c.min_m ? c.h[b].m : c.min_m;
  }
  static const long long budget = [] { const char* e = getenv("SPR_MATCH_GROUP_MB"); return (long long)(e ? atoi(e) : 250) << 20; }();
  const long long pair_bytes = (long long)c.max_n * c.max_m * 4;
  long long g = pair_bytes > 0 ? budget / pair_bytes : npairs;
  c.per_group = one_group ? npairs : (int)(g < 1 ? 1 : (g > npairs ? npairs : g));
  c.ngroups = cdiv(npairs, c.per_group);
  c.grouped = split && d % 32 == 0;
  c.gg = c.grouped ? cw.gg : nullptr;
  int bm = 1, bn = 1;
  if (c.grouped) gemm_group_tile(c.max_m, &bm, &bn);
  // descriptors are rebuilt on the device from cu (no pageable host copy)
  hipLaunchKernelGGL(k_build_pairs, dim3(1), dim3(64), 0, stream, cu_dev, npairs, c.pd, c.gg, d, bm, bn, c.per_group);
  // two range measurements serve every pair: all src tokens (A operands), all tgt tokens (B)
  c.sparts = c.tparts = nullptr;
  if (split) {
    float *ps = cw.sparts, *pt = cw.tparts;
    const int nsrc = cu_host[npairs], ntot = cu_host[2 * npairs];
    if (int rc = launch_absmax2(feat, nsrc, d, d, ps, feat + (size_t)nsrc * d, ntot - nsrc, d, d, pt, stream))
      return rc;
    c.sparts = ps;
    c.tparts = pt;
  }
  return 0;
}
int corr_gemm(const Corr& c, int g, int epi_mode, const float* epi, hipStream_t stream, bool* applied) {
  if (applied) *applied = false;
  const int p0 = c.first(g), np = c.count(g);
  if (c.grouped) {
    int bm, bn, tiles = 0;
    gemm_group_tile(c.max_m, &bm, &bn);
    for (int b = p0; b < p0 + np; ++b) tiles += cdiv(c.h[b].n, bm) * cdiv(c.h[b].m, bn);
    // one launch for the group: a 1 930 x 1 930 x 256 product alone is 64 tiles of 256 x 256, a quarter of the chip
    if (launch_gemm_grouped(c.feat, c.d, c.feat, c.mat, c.gg + p0, tiles, c.max_m, c.sparts, c.tparts, epi_mode, epi,
                            stream))
      return 1;
    if (applied) *applied = epi_mode != 0;
  } else {
    for (int b = p0; b < p0 + np; ++b)
      if (launch_linear_ranged(c.feat + (size_t)c.h[b].src_beg * c.d, c.h[b].n, c.d,
                               c.feat + (size_t)c.h[b].tgt_beg * c.d, c.h[b].m, nullptr, c.mat + c.h[b].off, c.sparts,
                               c.tparts, stream))
        return 1;
  }
  return 0;
}

// The matching head: dual-softmax matches (want_match) and / or Sinkhorn correspondences (want_sinkhorn) of one set
// of features.  The scaled correlation matrices are stored once per group (GEMM epilogue kEpiScale, or k_scale after
// the exact-f32 GEMMs); the Sinkhorn passes read them through the affinity view (struct Aff).  With both wanted, the
// dual softmax's row / column reduction and the first Sinkhorn iteration share a sweep where the two-quantity
// kernels (k_row_lse_v / k_col_lse_v with RAW) take the shape (same bits as the separate sweeps).  Every output is therefore bit for bit the same
// whichever entry point asked for it.
struct HeadArgs {
  const char* name;
  const float* feat;
  int d;
  const int *cu, *cu_host;
  int npairs;
  void* ws;
  size_t ws_bytes;
  hipStream_t stream;
  // what only one of the two heads reads (set by name in the entry points)
  const float* xyz = nullptr;
  const float *alpha = nullptr, *beta = nullptr;
  int n_iters = 0;
  float *match_val = nullptr, *match_val2 = nullptr;
  int* match_ind = nullptr;
  float *out_w = nullptr, *out_that = nullptr;
};
HeadArgs head_args(const char* name, const float* feat, int d, const int* cu, const int* cu_host, int npairs, void* ws,
                   size_t ws_bytes, void* stream) {
  HeadArgs a;
  a.name = name;
  a.feat = feat;
  a.d = d;
  a.cu = cu;
  a.cu_host = cu_host;
  a.npairs = npairs;
  a.ws = ws;
  a.ws_bytes = ws_bytes;
  a.stream = (hipStream_t)stream;
  return a;
}
int match_head(const HeadArgs& a, bool want_match, bool want_sinkhorn) {
  hipStream_t stream = a.stream;
  SPR_REQUIRE(a.npairs >= 1 && a.d % 32 == 0 && a.n_iters >= 0, "%s: need npairs >= 1, d %% 32 == 0, n_iters >= 0",
              a.name);
  const bool split = gemm_mode() == 1;
  Workspace w(a.ws, a.ws_bytes);
  const auto [epi, corr_ws, row_lse, col_lse, u, v] = head_layout(w, a.cu_host, a.npairs, split, want_match, want_sinkhorn);
  SPR_REQUIRE(a.ws != nullptr && w.ok(), "%s: workspace too small", a.name);
  const float scale = 1.0f / sqrtf((float)a.d);
  hipLaunchKernelGGL(k_epi_params, dim3(1), dim3(64), 0, stream, scale, want_sinkhorn ? a.alpha : nullptr,
                     want_sinkhorn ? a.beta : nullptr, epi);
  const float* aff = want_sinkhorn ? epi : nullptr;
  Corr c;
  if (corr_setup(c, a.feat, a.d, a.cu, a.cu_host, a.npairs, corr_ws, split, stream, false)) return 1;
  const int T = a.cu_host[2 * a.npairs];
  if (want_sinkhorn) {
    SPR_HIP_CHECK(hipMemsetAsync(u, 0, sizeof(float) * T, stream));
    SPR_HIP_CHECK(hipMemsetAsync(v, 0, sizeof(float) * T, stream));
  }
  // with both heads wanted the dual softmax's reductions and the first Sinkhorn iteration share their sweeps
  const bool fuse = want_match && want_sinkhorn && a.n_iters >= 1 && lse_raw_ok(c.max_m, c.min_m);
  for (int g = 0; g < c.ngroups; ++g) {
    bool scaled = false;
    if (corr_gemm(c, g, kEpiScale, epi, stream, &scaled)) return 1;
    const int np = c.count(g);
    const PairDesc* pg = c.pd + c.first(g);
    if (!scaled) {
      const long long cnt = c.end(g) - c.beg(g);
      hipLaunchKernelGGL(k_scale, dim3(cdiv(cnt, 256)), dim3(256), 0, stream, c.mat + c.beg(g), cnt, scale);
    }
    const dim3 grow(cdiv((long)c.max_n * 64, 256), np), gcol(cdiv(c.max_m, 64), np);
    if (fuse) {
      if (launch_row_lse<float>(c.mat, pg, np, c.max_n, c.max_m, u, (const float*)v, 1, stream, aff, row_lse)) return 1;
      if (launch_col_lse<float>(c.mat, pg, np, c.max_m, v, (const float*)u, 1, stream, c.min_m, aff, col_lse)) return 1;
    } else if (want_match) {
      launch_row_lse<float>(c.mat, pg, np, c.max_n, c.max_m, row_lse, nullptr, 0, stream);
      launch_col_lse<float>(c.mat, pg, np, c.max_m, col_lse, nullptr, 0, stream, c.min_m);
    }
    if (want_match) {
      hipLaunchKernelGGL(k_match_cols, gcol, dim3(1024), 0, stream, c.mat, pg, row_lse, col_lse, a.match_val,
                         a.match_ind, a.match_val2);
      hipLaunchKernelGGL(k_match_rows, grow, dim3(256), 0, stream, c.mat, pg, row_lse, col_lse, a.match_val,
                         a.match_ind, a.match_val2);
    }
    if (want_sinkhorn) {
      for (int it = fuse ? 1 : 0; it < a.n_iters; ++it) {
        launch_row_lse<float>(c.mat, pg, np, c.max_n, c.max_m, u, (const float*)v, 1, stream, aff);
        launch_col_lse<float>(c.mat, pg, np, c.max_m, v, (const float*)u, 1, stream, c.min_m, aff);
      }
      hipLaunchKernelGGL(k_sinkhorn_final, grow, dim3(256), 0, stream, c.mat, pg, u, v, a.xyz, a.out_w, a.out_that,
                         aff);
    }
  }
  SPR_LAUNCH_CHECK();
  return 0;
}
}  // namespace

extern "C" int spr_match_dualsoftmax(const float* feat, int d, const int* cu, const int* cu_host,
                                     int npairs, float* match_val, float* match_val2, int* match_ind, void* ws,
                                     size_t ws_bytes, void* stream_) {
  HeadArgs a = head_args("match", feat, d, cu, cu_host, npairs, ws, ws_bytes, stream_);
  a.match_val = match_val;
  a.match_val2 = match_val2;
  a.match_ind = match_ind;
  return match_head(a, true, false);
}

extern "C" int spr_pose_residuals(const float* pose, const float* a, const float* b, const int* pair_cu,
                                  int npairs, int total_host, float* res, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPR_REQUIRE(npairs >= 1 && total_host >= 1 && pose && a && b && pair_cu && res, "pose_residuals: bad arguments");
  hipLaunchKernelGGL(k_pose_residuals, dim3(cdiv(total_host, 256)), dim3(256), 0, stream, pose, a, b, pair_cu, npairs,
                     res);
  SPR_LAUNCH_CHECK();
  return 0;
}

extern "C" int spr_pose_scores(const float* poses, int nh, const float* a, const float* b, int n, float* score,
                               void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPR_REQUIRE(nh >= 1 && n >= 1 && poses && a && b && score, "pose_scores: bad arguments");
  hipLaunchKernelGGL(k_pose_scores, dim3(cdiv((long)nh * 64, 256)), dim3(256), 0, stream, poses, nh, a, b, n, score);
  SPR_LAUNCH_CHECK();
  return 0;
}

extern "C" int spr_sinkhorn_correspondences(const float* feat, int d, const float* xyz, const int* cu,
                                            const int* cu_host, int npairs, const float* alpha,
                                            const float* beta, int n_iters, int slack, float* out_w,
                                            float* out_that,
                                            void* ws, size_t ws_bytes, void* stream_) {
  (void)slack;  // the reference's sinkhorn() always pads the slack row/col (se3_torch.py:182-184)
  SPR_REQUIRE(alpha != nullptr && beta != nullptr, "sinkhorn: alpha / beta must be device pointers");
  HeadArgs a = head_args("sinkhorn", feat, d, cu, cu_host, npairs, ws, ws_bytes, stream_);
  a.xyz = xyz;
  a.alpha = alpha;
  a.beta = beta;
  a.n_iters = n_iters;
  a.out_w = out_w;
  a.out_that = out_that;
  return match_head(a, false, true);
}

// spr_match_dualsoftmax + spr_sinkhorn_correspondences of the SAME features in one call (what RegTR's inference
// forward runs back to back, qk_regtr_full.py:453-479 and :525-536).  Outputs are bit for bit those of the two
// separate calls.  match_val2 may be NULL.  Workspace: spr_match_workspace_bytes.
extern "C" int spr_match_sinkhorn(const float* feat, int d, const float* xyz, const int* cu, const int* cu_host,
                                  int npairs, const float* alpha, const float* beta, int n_iters, float* match_val,
                                  float* match_val2, int* match_ind, float* out_w, float* out_that, void* ws,
                                  size_t ws_bytes, void* stream_) {
  SPR_REQUIRE(feat && xyz && cu && cu_host && alpha && beta && match_val && match_ind && out_w && out_that,
              "match_sinkhorn: null argument");
  HeadArgs a = head_args("match_sinkhorn", feat, d, cu, cu_host, npairs, ws, ws_bytes, stream_);
  a.xyz = xyz;
  a.alpha = alpha;
  a.beta = beta;
  a.n_iters = n_iters;
  a.match_val = match_val;
  a.match_val2 = match_val2;
  a.match_ind = match_ind;
  a.out_w = out_w;
  a.out_that = out_that;
  return match_head(a, true, true);
}

extern "C" int spr_weighted_procrustes(const float* a, const float* b, const float* w,
                                       const int* pair_cu, int npairs, float* out_pose,
                                       void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPR_REQUIRE(npairs >= 1, "procrustes: npairs must be >= 1");
  hipLaunchKernelGGL(k_procrustes, dim3(npairs), dim3(256), 0, stream, a, b, w, pair_cu, out_pose);
  SPR_LAUNCH_CHECK();
  return 0;
}

// ---- backward entry points ---------------------------------------------------
extern "C" int spr_weighted_procrustes_bwd(const float* a, const float* b, const float* w, const int* pair_cu,
                                           int npairs, const float* dpose, float* da, float* db, float* dw,
                                           void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPR_REQUIRE(npairs >= 1 && a && b && pair_cu && dpose, "procrustes_bwd: bad arguments");
  SPR_REQUIRE(dw == nullptr || w != nullptr, "procrustes_bwd: dw needs w");
  hipLaunchKernelGGL(k_procrustes_bwd, dim3(npairs), dim3(256), 0, stream, a, b, w, pair_cu, dpose, da, db, dw);
  SPR_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t spr_sinkhorn_bwd_workspace_bytes(const int* cu_host, int npairs, int n_iters) {
  return measure(sinkhorn_bwd_layout, cu_host, npairs, n_iters, true);
}

// Gradient of (w, t_hat) = spr_sinkhorn_correspondences(feat, ...) w.r.t. feat, alpha, beta.
//   dw [Tsrc], dthat [Tsrc, 3] in;  dfeat [T, d] (written completely), dalpha [1], dbeta [1] out.
extern "C" int spr_sinkhorn_bwd(const float* feat, int d, const float* xyz, const int* cu, const int* cu_host,
                                int npairs, const float* alpha, const float* beta, int n_iters, const float* dw,
                                const float* dthat, float* dfeat, float* dalpha, float* dbeta, void* ws,
                                size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPR_REQUIRE(npairs >= 1 && d % 32 == 0 && n_iters >= 0, "sinkhorn_bwd: bad arguments");
  SPR_REQUIRE(feat && xyz && cu && cu_host && alpha && beta && dw && dthat && dfeat && dalpha && dbeta,
              "sinkhorn_bwd: null operand");
  const bool split = gemm_mode() == 1;
  Workspace w(ws, ws_bytes);
  const auto [corr_ws, corr, dmat, rs, rt, U, V, du, dva, dvb, zero, parts, epi] =
      sinkhorn_bwd_layout(w, cu_host, npairs, n_iters, split);
  SPR_REQUIRE(ws != nullptr && w.ok(), "sinkhorn_bwd: workspace too small");
  Corr c;
  if (corr_setup(c, feat, d, cu, cu_host, npairs, corr_ws, split, stream, true)) return 1;     // the backward keeps every matrix
  if (corr_gemm(c, 0, 0, nullptr, stream, nullptr)) return 1;
  const int T = cu_host[2 * npairs];
  const float scale = 1.0f / sqrtf((float)d);
  SPR_HIP_CHECK(hipMemsetAsync(dmat, 0, sizeof(float) * (size_t)c.total, stream));
  SPR_HIP_CHECK(hipMemcpyAsync(corr, c.mat, sizeof(float) * (size_t)c.total, hipMemcpyDeviceToDevice, stream));
  hipLaunchKernelGGL(k_epi_params, dim3(1), dim3(64), 0, stream, scale, alpha, beta, epi);
  hipLaunchKernelGGL(k_affinity, dim3(cdiv(c.total, 256)), dim3(256), 0, stream, c.mat, c.total, (const float*)epi);
  SPR_HIP_CHECK(hipMemsetAsync(zero, 0, sizeof(double) * T, stream));
  const dim3 grow(cdiv((long)c.max_n * 64, 256), npairs), gcol(cdiv(c.max_m, 64), npairs);
  // forward potentials, every iteration kept
  for (int it = 0; it < n_iters; ++it) {
    double* ut = U + (size_t)it * T;
    const double* vprev = it == 0 ? zero : V + (size_t)(it - 1) * T;
    launch_row_lse<double>(c.mat, c.pd, npairs, c.max_n, c.max_m, ut, vprev, 1, stream);
    launch_col_lse<double>(c.mat, c.pd, npairs, c.max_m, V + (size_t)it * T, (const double*)ut, 1, stream, c.min_m);
  }
  const double* un = n_iters > 0 ? U + (size_t)(n_iters - 1) * T : zero;
  const double* vn = n_iters > 0 ? V + (size_t)(n_iters - 1) * T : zero;
  // final step: dA = gP * P, du_n, dv_n
  hipLaunchKernelGGL(k_sk_bwd_final, grow, dim3(256), 0, stream, c.mat, dmat, c.pd, un, vn, xyz, dw, dthat, du);
  hipLaunchKernelGGL(k_sk_colsum_neg, gcol, dim3(1024), 0, stream, dmat, c.pd, dva);
  float* dv_cur = dva;
  float* dv_prev = dvb;
  for (int it = n_iters - 1; it >= 0; --it) {
    const double* ut = U + (size_t)it * T;
    const double* vt = V + (size_t)it * T;
    // v_t = colLSE(A - u_t): adds to dA and to du_t
    hipLaunchKernelGGL(k_sk_bwd_col, grow, dim3(256), 0, stream, c.mat, dmat, c.pd, ut, vt, (const float*)dv_cur, du);
    // u_t = rowLSE(A - v_{t-1}): adds to dA, produces dv_{t-1} (v_0 = 0 is a constant)
    const double* vprev = it == 0 ? nullptr : V + (size_t)(it - 1) * T;
    hipLaunchKernelGGL(k_sk_bwd_row, gcol, dim3(1024), 0, stream, c.mat, dmat, c.pd, ut, vprev, (const float*)du,
                       it == 0 ? (float*)nullptr : dv_prev);
    if (it > 0) {
      // du_{t-1} starts from zero: only v_{t-1} depends on it
      SPR_HIP_CHECK(hipMemsetAsync(du, 0, sizeof(float) * T, stream));
      float* t = dv_cur;
      dv_cur = dv_prev;
      dv_prev = t;
    }
  }
  // affinity -> correlation, alpha, beta
  const int nparts = 1024;
  hipLaunchKernelGGL(k_affinity_bwd, dim3(nparts), dim3(256), 0, stream, corr, c.mat, dmat, c.total, scale, beta, parts);
  hipLaunchKernelGGL(k_affinity_bwd_final, dim3(1), dim3(64), 0, stream, parts, nparts, alpha, beta, dalpha, dbeta);
  // correlation -> features: dFs = dcorr Ft, dFt = dcorr^T Fs (exact-f32 batched GEMM)
  hipLaunchKernelGGL(k_build_grad_recs, dim3(cdiv(npairs, 64)), dim3(64), 0, stream, c.pd, npairs, d, rs, rt);
  SPR_LAUNCH_CHECK();
  // all pairs in one launch per product: the records carry each pair's own leading dimension (BgemmDesc.pad), a
  // pair alone is 38 tiles of 128 x 128
  if (int rc = spr_bgemm(dmat, feat, dfeat, rs, npairs, c.max_n, d, c.max_m, 1, d, 1, d, 1, 1.0f, 0.0f, stream_)) return rc;
  if (int rc = spr_bgemm(dmat, feat, dfeat, rt, npairs, c.max_m, d, 1, c.max_m, d, 1, d, 1, 1.0f, 0.0f, stream_)) return rc;
  return 0;
}
