// a9, analysis -- the softmax attention maps of the varlen multi-head core on gfx950.
//
// Behaviour contract: the attention weights nn.MultiheadAttention returns with need_weights=True
// (averaged over the heads by default) for the four calls per layer of TransformerCrossEncoderLayer
//   models/transformer/transformers.py:198-227 (pre-norm), :133-165 (post-norm),
// stored at :179-180 / :242-243 and stacked by TransformerCrossEncoder.get_attentions (:61-82):
//   P_h[i, j] = softmax_j(scale q_i,h . k_j,h),   segment s attends to segment kv_seg[s].
// The reference's key padding mask becomes the segment bounds; entries outside a segment's Lq x Lk
// block of the caller's padded output are written as exact zeros.
//
// The arithmetic is independent of the attention core's mode (spr_set_attn_mode): this file carries
// its own split-fp16 Q / K planes and its own fp32 row statistics.
//   k_probs_pack    Q (pre-scaled by log2(e) scale) and K as fp16 hi + lo planes, head-major
//                   [head][token][32], with the range balancing of attention.hip (K 2^ek, Q 2^-ek:
//                   both planes sit at sqrt(|q||k|)), so no magnitude leaves fp16's range.
//   k_probs_stats   pass 1: per query and head the row maximum m and 1 / sum_j 2^(s_j - m) in fp32,
//                   S^T = K Q^T with v_mfma_f32_32x32x16_f16 (hh + hl + lh), lane = query; every
//                   half-wave keeps an online (max, sum) over its 16 keys of a tile, joined at the end.
//   k_probs_write   pass 2: recomputes the scores (the same instructions, hence the same bits as pass 1),
//                   p = 2^(s - m) / l, the head mean accumulated in registers (no atomics), staged
//                   through LDS and written as rows with 16-byte stores (4 rows x 256 bytes per wave
//                   instruction).  Fixed summation order everywhere: bitwise reproducible.
#include "spr_common.h"
#include "split_mma.h"

namespace spr {
namespace {

constexpr int HD = 32;         // head dim
constexpr int QB = 128;        // queries per workgroup (4 waves x 32)
constexpr int KR = 64;         // keys per workgroup of the store pass (2 sub-tiles of 32)
constexpr int LSR = KR + 4;    // LDS row stride (floats) of the store staging: 16-byte rows 4 banks apart

// scales[0] = log2(e) scale 2^-ek (Q planes), scales[1] = 2^ek (K planes), ek = half the exponent gap of the bounds
__global__ __launch_bounds__(256) void k_probs_scales(const float* __restrict__ q_parts,
                                                      const float* __restrict__ k_parts, float qscale,
                                                      float* __restrict__ scales) {
  __shared__ float sh[17];
  const float qb = block_absmax(q_parts, sh) * qscale;
  const float kb = block_absmax(k_parts, sh);
  if (threadIdx.x == 0) {
    int ek = 0;
    if (qb > 0.f && kb > 0.f && qb < 3.0e38f && kb < 3.0e38f) {
      const int eq = (int)((__float_as_uint(qb) >> 23) & 0xff) - 127;
      const int ekk = (int)((__float_as_uint(kb) >> 23) & 0xff) - 127;
      ek = max(-60, min(60, (eq - ekk) >> 1));
    }
    scales[0] = qscale * pow2f(-ek);
    scales[1] = pow2f(ek);
  }
}

// one thread = 4 features of one token of q and of k
__global__ __launch_bounds__(256) void k_probs_pack(const float* __restrict__ q, int q_stride,
                                                    const float* __restrict__ k, int k_stride, int t_total,
                                                    int d_model, const float* __restrict__ scales,
                                                    _Float16* __restrict__ qh, _Float16* __restrict__ ql,
                                                    _Float16* __restrict__ kh, _Float16* __restrict__ kl) {
  const int d4 = d_model / 4;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)t_total * d4) return;
  const int tok = (int)(i / d4), f = (int)(i % d4) * 4;
  const float4 vq = *reinterpret_cast<const float4*>(q + (size_t)tok * q_stride + f);
  const float4 vk = *reinterpret_cast<const float4*>(k + (size_t)tok * k_stride + f);
  const size_t hm = ((size_t)(f / HD) * t_total + tok) * HD + f % HD;
  split_store4(vq, scales[0], qh + hm, ql + hm);
  split_store4(vk, scales[1], kh + hm, kl + hm);
}

// Block id -> (group, tile) with all tiles of one group on one XCD (ids b and b + 8 share an L2) when the group
// count allows it, as k_attn_s does.
__device__ __forceinline__ void group_tile(int b, int ngrp, int ntile, int& g, int& tile) {
  if ((ngrp & 7) == 0) {
    const int xcd = b & 7, idx = b >> 3;
    g = xcd + 8 * (idx / ntile);
    tile = idx % ntile;
  } else {
    g = b / ntile;
    tile = b % ntile;
  }
}

// S^T = K Q^T of one 32-key x 32-query sub-tile in split fp16 (rows = keys, lane = query), C = c0.
__device__ __forceinline__ f32x16 scores_t(const _Float16* __restrict__ kh_g, const _Float16* __restrict__ kl_g,
                                           size_t krow, const f16x8 (&qh)[2], const f16x8 (&ql)[2], f32x16 c) {
  f16x8 kfh[2], kfl[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    kfh[s] = *reinterpret_cast<const f16x8*>(kh_g + krow + 16 * s);
    kfl[s] = *reinterpret_cast<const f16x8*>(kl_g + krow + 16 * s);
  }
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    c = mma3_32(kfh[s], kfl[s], qh[s], ql[s], c);
  }
  return c;
}

__device__ __forceinline__ void load_q(const _Float16* __restrict__ qh_g, const _Float16* __restrict__ ql_g,
                                       size_t row, f16x8 (&qh)[2], f16x8 (&ql)[2]) {
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    qh[s] = *reinterpret_cast<const f16x8*>(qh_g + row + 16 * s);
    ql[s] = *reinterpret_cast<const f16x8*>(ql_g + row + 16 * s);
  }
}

constexpr float kNegBig = -3.0e38f;   // running maximum before the first valid key (finite: no inf - inf)

// Pass 1.  Grid: nseg x nhead groups x ceil(max_len / 128) query tiles; m_out / rl_out [nhead][t].
__global__ __launch_bounds__(256) void k_probs_stats(const _Float16* __restrict__ qh_g,
                                                     const _Float16* __restrict__ ql_g,
                                                     const _Float16* __restrict__ kh_g,
                                                     const _Float16* __restrict__ kl_g, int t_total,
                                                     const int* __restrict__ cu, const int* __restrict__ kv_seg,
                                                     int nseg, int nhead, int nqt, float* __restrict__ m_out,
                                                     float* __restrict__ rl_out) {
  int g, qt;
  group_tile(blockIdx.x, nseg * nhead, nqt, g, qt);
  const int seg = g / nhead, head = g % nhead;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l31 = lane & 31, lh = lane >> 5;
  const int qbeg = cu[seg], qlen = cu[seg + 1] - qbeg;
  const int q0 = qt * QB + wave * 32;
  if (q0 >= qlen) return;
  const int ks = kv_seg[seg];
  const int kbeg = cu[ks], klen = cu[ks + 1] - kbeg;
  f16x8 qh[2], ql[2];
  load_q(qh_g, ql_g, ((size_t)head * t_total + qbeg + min(q0 + l31, qlen - 1)) * HD + 8 * lh, qh, ql);
  float m = kNegBig, l = 0.f;
  for (int kt = 0; kt < klen; kt += 64) {   // two 32-key sub-tiles per step: both fragment loads in flight at once
    f32x16 sc[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const size_t krow = ((size_t)head * t_total + kbeg + min(kt + 32 * kk + l31, klen - 1)) * HD + 8 * lh;
      sc[kk] = (f32x16){};
      sc[kk] = scores_t(kh_g, kl_g, krow, qh, ql, sc[kk]);
    }
    if (kt + 64 > klen) {
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (acc_row32(r, lh, kt + 32 * kk) >= klen) sc[kk][r] = -INFINITY;
    }
    float mx = fmaxf(sc[0][0], sc[1][0]);
#pragma unroll
    for (int r = 1; r < 16; ++r) mx = fmaxf(mx, fmaxf(sc[0][r], sc[1][r]));
    const float mn = fmaxf(m, mx);
    float ts = 0.f;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int r = 0; r < 16; ++r) ts += __builtin_amdgcn_exp2f(sc[kk][r] - mn);
    l = l * __builtin_amdgcn_exp2f(m - mn) + ts;
    m = mn;
  }
  // join the two half-waves (keys 4 h + 8 i + (0..3) of every tile)
  const float mo = __shfl_xor(m, 32, 64), lo = __shfl_xor(l, 32, 64);
  const float mm = fmaxf(m, mo);
  const float ll = l * __builtin_amdgcn_exp2f(m - mm) + lo * __builtin_amdgcn_exp2f(mo - mm);   // used by lh == 0
  if (lh == 0 && q0 + l31 < qlen) {
    const size_t o = (size_t)head * t_total + qbeg + q0 + l31;
    m_out[o] = mm;
    rl_out[o] = ll > 0.f ? 1.0f / ll : 0.f;
  }
}

// Pass 2.  Grid: nseg x ceil(max_cols / 64) groups x ceil(max_rows / 128) query tiles (all query tiles of one
// (segment, key range) on one XCD).  place [nseg][5] = {element offset, row stride, head stride, rows, cols}:
// segment s owns rows x cols entries (per head) at out + off (+ h head_stride); the Lq x Lk block of
// probabilities sits in its top-left corner, everything else is written as 0.
template <bool PER_HEAD>
__global__ __launch_bounds__(256) void k_probs_write(const _Float16* __restrict__ qh_g,
                                                     const _Float16* __restrict__ ql_g,
                                                     const _Float16* __restrict__ kh_g,
                                                     const _Float16* __restrict__ kl_g, int t_total,
                                                     const int* __restrict__ cu, const int* __restrict__ kv_seg,
                                                     int nseg, int nhead, int nkr, int nqt,
                                                     const float* __restrict__ m_in, const float* __restrict__ rl_in,
                                                     float* __restrict__ out, const long long* __restrict__ place) {
  __shared__ __align__(16) float stage[4][32 * LSR];
  int g, qt;
  group_tile(blockIdx.x, nseg * nkr, nqt, g, qt);
  const int seg = g / nkr, kr = g % nkr;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l31 = lane & 31, lh = lane >> 5;
  const long long* pl = place + 5 * (size_t)seg;
  const long long off = pl[0], ld = pl[1], hstride = pl[2];
  const int rows = (int)pl[3], cols = (int)pl[4];
  const int q0 = qt * QB + wave * 32, k0 = kr * KR;
  if (q0 >= rows || k0 >= cols) return;
  const int qbeg = cu[seg], qlen = cu[seg + 1] - qbeg;
  const int ks = kv_seg[seg];
  const int kbeg = cu[ks], klen = cu[ks + 1] - kbeg;
  const bool live = q0 < qlen && k0 < klen;   // wave-uniform: else the wave writes zeros only
  const bool qvalid = q0 + l31 < qlen;
  const int qi = min(q0 + l31, qlen - 1);
  float* st = stage[wave];
  float* const base = out + off;
  const bool vec = ((reinterpret_cast<uintptr_t>(base) & 15) == 0) && (ld & 3) == 0 && (!PER_HEAD || (hstride & 3) == 0);

  f32x16 acc[2];
  auto zero = [&]() {
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[kk][r] = 0.f;
  };
  // p = 2^(s - m) / l of one head, added to acc
  auto head_probs = [&](int head) {
    f16x8 qh[2], ql[2];
    const size_t qrow = (size_t)head * t_total + qbeg + qi;
    load_q(qh_g, ql_g, qrow * HD + 8 * lh, qh, ql);
    const float m = m_in[qrow], rl = rl_in[qrow];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int kt = k0 + 32 * kk;   // a sub-tile past klen reads the last key and is masked below (no branch)
      const size_t krow = ((size_t)head * t_total + kbeg + min(kt + l31, klen - 1)) * HD + 8 * lh;
      f32x16 c = {};
      c = scores_t(kh_g, kl_g, krow, qh, ql, c);   // bitwise the scores of pass 1: rows sum to 1 to rounding
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float p = __builtin_amdgcn_exp2f(c[r] - m);
        const bool kvalid = acc_row32(r, lh, kt) < klen;
        acc[kk][r] = kvalid ? fmaf(p, rl, acc[kk][r]) : acc[kk][r];
      }
    }
  };
  // acc (lane = query row l31, keys 32 kk + 8 i + 4 lh + (0..3)) -> LDS rows -> 16-byte row stores
  auto store = [&](float* dst, float mul) {
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float4 v = make_float4(acc[kk][4 * i] * mul, acc[kk][4 * i + 1] * mul, acc[kk][4 * i + 2] * mul,
                               acc[kk][4 * i + 3] * mul);
        if (!qvalid) v = make_float4(0.f, 0.f, 0.f, 0.f);
        *reinterpret_cast<float4*>(st + l31 * LSR + 32 * kk + 8 * i + 4 * lh) = v;
      }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the wave's staging is private: in-order LDS suffices
    const int c = k0 + 4 * (lane & 15);
#pragma unroll 2
    for (int it = 0; it < 8; ++it) {
      const int row = 4 * it + (lane >> 4);
      if (q0 + row >= rows) break;
      const float4 v = *reinterpret_cast<const float4*>(st + row * LSR + 4 * (lane & 15));
      float* d = dst + (size_t)(q0 + row) * ld;
      if (vec && c + 4 <= cols) {
        *reinterpret_cast<float4*>(d + c) = v;
      } else {
        if (c < cols) d[c] = v.x;
        if (c + 1 < cols) d[c + 1] = v.y;
        if (c + 2 < cols) d[c + 2] = v.z;
        if (c + 3 < cols) d[c + 3] = v.w;
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // reads done before the next head's staging
  };

  if constexpr (PER_HEAD) {
    for (int h = 0; h < nhead; ++h) {
      zero();
      if (live) head_probs(h);
      store(base + (size_t)h * hstride, 1.0f);
    }
  } else {
    zero();
    if (live) {
#pragma unroll 2
      for (int h = 0; h < nhead; ++h) head_probs(h);
    }
    store(base, 1.0f / (float)nhead);
  }
}

}  // namespace
}  // namespace spr

using namespace spr;

namespace {
struct ProbsWs {
  _Float16 *qh, *ql, *kh, *kl;
  float *m, *rl, *qparts, *kparts, *scales;
};
ProbsWs probs_layout(Workspace& a, int t, int nhead) {
  const size_t n = (size_t)t * nhead * HD;
  ProbsWs w;
  w.qh = a.take<_Float16>(n);
  w.ql = a.take<_Float16>(n);
  w.kh = a.take<_Float16>(n);
  w.kl = a.take<_Float16>(n);
  w.m = a.take<float>((size_t)t * nhead);
  w.rl = a.take<float>((size_t)t * nhead);
  w.qparts = a.take<float>(kAmaxParts);
  w.kparts = a.take<float>(kAmaxParts);
  w.scales = a.take<float>(4);
  return w;
}
}  // namespace

extern "C" size_t spr_attn_probs_workspace_bytes(int t, int nhead, int head_dim) {
  if (t < 1 || nhead < 1 || head_dim != HD) return 0;
  return measure(probs_layout, t, nhead);
}

extern "C" int spr_attn_probs(const float* q, int q_stride, const float* k, int k_stride, const int* cu,
                              const int* kv_seg, int t, int nseg, int max_len_host, int nhead, int head_dim,
                              float scale, int per_head, float* out, const long long* place, int max_rows_host,
                              int max_cols_host, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPR_REQUIRE(head_dim == HD, "attention probs: head_dim must be %d (got %d)", HD, head_dim);
  SPR_REQUIRE(q && k && cu && kv_seg && out && place && ws, "attention probs: null pointer argument");
  SPR_REQUIRE(nseg >= 1, "attention probs: nseg must be >= 1 (got %d)", nseg);
  SPR_REQUIRE(t >= 1 && nhead >= 1 && max_len_host >= 1 && max_rows_host >= 1 && max_cols_host >= 1,
              "attention probs: bad sizes (t=%d nhead=%d max_len=%d max_rows=%d max_cols=%d)", t, nhead, max_len_host,
              max_rows_host, max_cols_host);
  SPR_REQUIRE(q_stride % 4 == 0 && k_stride % 4 == 0 && q_stride >= nhead * HD && k_stride >= nhead * HD &&
                  ((uintptr_t)q & 15) == 0 && ((uintptr_t)k & 15) == 0,
              "attention probs: q / k rows must be 16-byte aligned with strides >= nhead * 32 (multiples of 4 floats)");
  Workspace a(ws, ws_bytes);
  const ProbsWs w = probs_layout(a, t, nhead);
  SPR_REQUIRE(a.ok(), "attention probs: workspace too small (%zu bytes given)", ws_bytes);
  const long nqt1 = cdiv(max_len_host, QB), nqt2 = cdiv(max_rows_host, QB), nkr = cdiv(max_cols_host, KR);
  SPR_REQUIRE(nqt1 * nhead * nseg < (1l << 31) && nqt2 * nkr * nseg < (1l << 31), "attention probs: grid too large");
  const int d = nhead * HD;
  if (int rc = launch_absmax2(q, t, d, q_stride, w.qparts, k, t, d, k_stride, w.kparts, stream)) return rc;
  hipLaunchKernelGGL(k_probs_scales, dim3(1), dim3(256), 0, stream, w.qparts, w.kparts, scale * 1.4426950408889634f,
                     w.scales);
  hipLaunchKernelGGL(k_probs_pack, dim3(cdiv((long)t * (d / 4), 256)), dim3(256), 0, stream, q, q_stride, k, k_stride,
                     t, d, w.scales, w.qh, w.ql, w.kh, w.kl);
  hipLaunchKernelGGL(k_probs_stats, dim3((unsigned)(nqt1 * nhead * nseg)), dim3(256), 0, stream, w.qh, w.ql, w.kh,
                     w.kl, t, cu, kv_seg, nseg, nhead, (int)nqt1, w.m, w.rl);
  const dim3 grid((unsigned)(nqt2 * nkr * nseg));
  if (per_head)
    hipLaunchKernelGGL(k_probs_write<true>, grid, dim3(256), 0, stream, w.qh, w.ql, w.kh, w.kl, t, cu, kv_seg, nseg,
                       nhead, (int)nkr, (int)nqt2, w.m, w.rl, out, place);
  else
    hipLaunchKernelGGL(k_probs_write<false>, grid, dim3(256), 0, stream, w.qh, w.ql, w.kh, w.kl, t, cu, kv_seg, nseg,
                       nhead, (int)nkr, (int)nqt2, w.m, w.rl, out, place);
  SPR_LAUNCH_CHECK();
  return 0;
}
