// a9 -- varlen multi-head attention core (flash style, exact f32) on gfx950.
//
// Behaviour contract: the scaled-dot-product core of nn.MultiheadAttention as
// called four times per layer in TransformerCrossEncoderLayer.forward_pre
//   /root/reference/src/models/transformer/transformers.py:198-227
// (softmax(Q K^T / sqrt(head_dim)) V per head, key padding mask = padded
// positions excluded, dropout 0).  The reference pads every sequence to the
// batch maximum and materialises (B*heads, Lq, Lk) weights; here tokens stay
// packed, segment s reads the keys/values of segment kv_seg[s] (itself for
// self attention, the partner cloud for cross attention) and nothing of size
// Lq x Lk ever reaches memory.
//
// Kernel shape (head_dim = 32):
//   workgroup = 4 waves = 128 queries of one (segment, head); each wave owns
//   32 queries.  S^T = K Q^T is computed with v_mfma_f32_32x32x2_f32 so that
//   a query is a LANE: the softmax row reductions are in-register (16
//   accumulator registers + one cross-half shuffle), and the probabilities in
//   the accumulator are already the B operand of O^T = V^T P^T with the key
//   order permuted consistently on both operands -- no LDS round trip for P.
//   K / V tiles of 32 keys are staged in LDS (row stride 33 / 32 words ->
//   conflict-free fragment reads) and shared by the four waves.
#include "attn_planes.h"
#include "lds_dma.h"
#include "spr_common.h"
#include "split_mma.h"
#include <atomic>
#include <type_traits>

namespace spr {
namespace {

constexpr int HD = 32;        // head dim
constexpr int KT = 32;        // keys per tile
constexpr int QW = 32;        // queries per wave
constexpr int QB = 128;       // queries per workgroup
constexpr int KS = HD + 1;    // K tile row stride (words)

__global__ __launch_bounds__(256) void k_attn(
    const float* __restrict__ q, int q_stride, const float* __restrict__ k, int k_stride,
    const float* __restrict__ v, int v_stride, const int* __restrict__ cu,
    const int* __restrict__ kv_seg, int nseg, int nhead, float scale, float* __restrict__ out,
    int o_stride) {
  // two LDS stages: tile t+1 is written while tile t is being read; one barrier per tile
  __shared__ float Ks[2][KT * KS];
  __shared__ float Vs[2][KT * HD];
  // 1-D grid: all query tiles of one (segment, head) -- which stream the same
  // K/V -- are placed on one XCD (ids b and b+8 share an L2)
  int seg, head, qt;
  {
    const int nqt = gridDim.x / (nhead * nseg);
    const int ngrp = nhead * nseg;
    const int b = blockIdx.x;
    if ((ngrp & 7) == 0) {
      const int xcd = b & 7, idx = b >> 3;
      const int g = xcd + 8 * (idx / nqt);
      qt = idx % nqt;
      head = g % nhead;
      seg = g / nhead;
    } else {
      qt = b % nqt;
      head = (b / nqt) % nhead;
      seg = b / (nqt * nhead);
    }
  }
  const int qbeg = cu[seg], qlen = cu[seg + 1] - qbeg;
  const int q0 = qt * QB;
  if (q0 >= qlen) return;  // uniform for the workgroup
  const int ks = kv_seg[seg];
  const int kbeg = cu[ks], klen = cu[ks + 1] - kbeg;

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int l31 = lane & 31, lh = lane >> 5;
  const int qi = q0 + wave * QW + l31;  // this lane's query (local index)
  const bool qok = qi < qlen;
  const int hoff = head * HD;

  // Q^T as B operand of S^T = K Q^T:  B[k = d][col = query]; step s covers
  // d = 2s + lh.  Pre-scaled by log2(e)/sqrt(head_dim): softmax runs in base 2
  // (v_exp_f32 is a base-2 exponential), mathematically identical.
  float qreg[16];
  {
    const float sc = scale * 1.4426950408889634f;
    const float* qp = q + (size_t)(qbeg + (qok ? qi : 0)) * q_stride + hoff;
#pragma unroll
    for (int s = 0; s < 16; ++s) qreg[s] = qok ? qp[2 * s + lh] * sc : 0.f;
  }

  f32x16 o;  // O^T[d][query]: lane = query, d = (r&3) + 8*(r>>2) + 4*lh
#pragma unroll
  for (int r = 0; r < 16; ++r) o[r] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;

  // staging role of this thread: key row sr (0..31), 4 dims starting at sc4
  const int sr = tid >> 3, sc4 = (tid & 7) * 4;
  f32x4 kreg, vreg;
  // The prefetch must stay in flight across the MFMA block; hipcc sinks plain
  // loads to their first use, so the two loads are issued by inline asm and
  // retired by an explicit s_waitcnt (nothing else is on the vector-memory
  // queue inside the loop).
  auto fetch = [&](int kt) {
    const int r = min(kt + sr, klen - 1);          // clamp: always a valid row
    const size_t row = (size_t)(kbeg + r);
    const float* kp_ = k + row * k_stride + hoff + sc4;
    const float* vp_ = v + row * v_stride + hoff + sc4;
    asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(kreg) : "v"(kp_));
    asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(vreg) : "v"(vp_));
  };
  auto stash = [&](int kt, int buf) {
    wait_vm<0>();
    __builtin_amdgcn_sched_barrier(0);
    const bool in = kt + sr < klen;                // rows past the segment read as zero
    float* kd = Ks[buf] + sr * KS + sc4;
    kd[0] = in ? kreg[0] : 0.f;
    kd[1] = in ? kreg[1] : 0.f;
    kd[2] = in ? kreg[2] : 0.f;
    kd[3] = in ? kreg[3] : 0.f;
    f32x4 vz = {in ? vreg[0] : 0.f, in ? vreg[1] : 0.f, in ? vreg[2] : 0.f, in ? vreg[3] : 0.f};
    *reinterpret_cast<f32x4*>(Vs[buf] + sr * HD + sc4) = vz;
  };

  if (klen > 0) {
    fetch(0);
    stash(0, 0);
  }
  __syncthreads();

  int buf = 0;
  for (int kt = 0; kt < klen; kt += KT, buf ^= 1) {
    const bool more = kt + KT < klen;
    if (more) fetch(kt + KT);
    __builtin_amdgcn_sched_barrier(0);

    // S^T tile: rows = keys, cols = queries.  A[row = key l31][k = d = 2s+lh]
    f32x16 st;
#pragma unroll
    for (int r = 0; r < 16; ++r) st[r] = 0.f;
    // all 16 A fragments are read from LDS up front (one exposed LDS latency
    // per tile instead of one per MFMA pair); V fragments are fetched before
    // the softmax so their latency hides under the VALU work.
    const float* kp = Ks[buf] + l31 * KS + lh;
    const float* vp = Vs[buf] + l31;
    float ka[16], va[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) ka[s] = kp[2 * s];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int s = 0; s < 16; ++s)
      st = __builtin_amdgcn_mfma_f32_32x32x2f32(ka[s], qreg[s], st, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 16; ++r) va[r] = vp[acc_row32(r, lh, 0) * HD];
    __builtin_amdgcn_sched_barrier(0);

    // lane holds, for its query, the 16 keys  j(r) = (r&3) + 8*(r>>2) + 4*lh
    float mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int j = acc_row32(r, lh, kt);
      if (j >= klen) st[r] = -INFINITY;  // tail of the key segment
      mx = fmaxf(mx, st[r]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));  // other half-lane: other 16 keys
    const float m_new = fmaxf(m_run, mx);    // finite: every tile has >= 1 key
    const float corr = __builtin_amdgcn_exp2f(m_run - m_new);
    float psum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      st[r] = __builtin_amdgcn_exp2f(st[r] - m_new);
      psum += st[r];
    }
    psum += __shfl_xor(psum, 32, 64);
    l_run = l_run * corr + psum;
    m_run = m_new;
#pragma unroll
    for (int r = 0; r < 16; ++r) o[r] *= corr;

    // O^T += V^T P^T.  Step r: lane half h contributes key j0(r) + 4h with
    // j0(r) = (r&3) + 8*(r>>2); B operand = st[r] (already in place),
    // A[row = d = l31][k = h] = V[j0(r) + 4h][d].
#pragma unroll
    for (int r = 0; r < 16; ++r)
      o = __builtin_amdgcn_mfma_f32_32x32x2f32(va[r], st[r], o, 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
    if (more) stash(kt + KT, buf ^ 1);
    __syncthreads();
  }

  if (qok) {
    const float inv = l_run > 0.f ? 1.f / l_run : 0.f;
    float* op = out + (size_t)(qbeg + qi) * o_stride + hoff;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      // registers 4g..4g+3 -> d = 8g + 4*lh + (0..3): one float4
      float4 w4 = make_float4(o[4 * g] * inv, o[4 * g + 1] * inv, o[4 * g + 2] * inv,
                              o[4 * g + 3] * inv);
      *reinterpret_cast<float4*>(op + 8 * g + 4 * lh) = w4;
    }
  }
}

// ---------------------------------------------------------------------------
// Split-fp16 variant: fp32-level accuracy, ~5x less matrix-core time.
// Every operand x is carried as hi = fp16(x m) and lo = fp16(x m - hi) with a
// per-tensor multiplier m (below); a.b ~= ah.bh + ah.bl + al.bh in ONE fp32
// accumulator (the matrix cores honour fp16 subnormals, scripts/abl/denorm.hip).
//
// Range safety (k_plane_scales): K is multiplied by 2^ek and Q by
// log2(e)/sqrt(d) 2^-ek with ek = half the exponent gap between the bounds of
// |q| and |k| -- the scores are unchanged, both planes sit at sqrt(|q||k|) and
// cannot overflow unless the scores themselves exceed 2^30; V is multiplied by
// 2^ev (max |v| 2^ev in [2^14, 2^15)) and the output by 2^-ev.  The bounds are
// measured (unfused entry: launch_absmax on q, k, v) or derived (fused entry:
// max|x| * max row L1 norm of the projection block + max|bias|).
// Mode 2 runs the same kernel with the hi planes only: single-pass fp16
// operands (11 significand bits), fp32 softmax and accumulators, 1/3 of the MFMAs.
//
// Two kernels:
//   k_attn_pack  splits Q (pre-scaled by log2(e)/sqrt(d)), K and V ONCE per
//     call into fp16 hi/lo planes in the workspace.  V is written TRANSPOSED
//     ([feature][token column]) because the V^T A-fragment of O^T = V^T P^T
//     wants 4 consecutive keys of one feature.  Token columns of segment s
//     start at vstart(s) = (cu[s] + 8 s) & ~7 (16-byte aligned rows for the
//     wide loads); gap and tail columns are written as zeros.
//   k_attn_s     streams 64-key tiles of those planes through LDS (LDS-DMA,
//     no conversion in the loop) and runs, per wave of 32 queries:
//       S^T = K Q^T : 2 key sub-tiles x 2 k-steps x 3 v_mfma_f32_32x32x16_f16
//       online softmax, lane = query, base 2, lazy reference (the row maximum
//         sits at 2^4 after a recentring), hi by packed conversion, lo by
//         v_fma_mix*_f16
//       O^T = V^T P^T: the probabilities in the S^T accumulator are converted
//         in place -- registers 8s..8s+7 of a lane are exactly the B fragment
//         of k-step s with key order kappa(s,h,j) = 16s + 8(j>>2) + 4h + (j&3);
//         the V^T A-fragment is read with the same order.
constexpr int KT2 = 64;  // keys per tile (two 32-key MFMA sub-tiles)
constexpr int PT = 64;   // token columns per pack workgroup
constexpr int PS = 72;   // pack transposition row stride (halves)

__device__ __forceinline__ int vstart(const int* __restrict__ cu, int s) {
  return attn_vstart_of(cu[s], s);
}

// Zeroes the gap columns between segments and the tail of the transposed V planes
// (written by k_attn_pack itself on the unfused path; needed when the in-projection
// GEMM emits the planes).  One workgroup per plane row.
__global__ __launch_bounds__(256) void k_attn_zero_gaps(const int* __restrict__ cu, int nseg, int tp,
                                                         _Float16* __restrict__ vth,
                                                         _Float16* __restrict__ vtl) {
  const int f = blockIdx.x, d = gridDim.x;
  for (int s = 0; s < nseg; ++s) {
    const int beg = vstart(cu, s) + cu[s + 1] - cu[s];
    const int end = s + 1 < nseg ? vstart(cu, s + 1) : tp;
    for (int c = beg + threadIdx.x; c < end; c += 256) {
      vth[attn_v_off(f, attn_vperm(c), d)] = (_Float16)0.f;     // (a bijection inside every aligned 16-column group)
      vtl[attn_v_off(f, attn_vperm(c), d)] = (_Float16)0.f;
    }
  }
}

// One workgroup = PT token columns x all features.  tp = padded column count.
__global__ __launch_bounds__(256) void k_attn_pack(
    const float* __restrict__ q, int q_stride, const float* __restrict__ k, int k_stride,
    const float* __restrict__ v, int v_stride, const int* __restrict__ cu, int nseg, int d_model,
    int t_total, int tp, const float* __restrict__ scales, _Float16* __restrict__ qh,
    _Float16* __restrict__ ql, _Float16* __restrict__ kh, _Float16* __restrict__ kl,
    _Float16* __restrict__ vth, _Float16* __restrict__ vtl) {
  const float qmul = scales[0], kmul = scales[1], vmul = scales[2];
  __shared__ __align__(16) _Float16 Lh[128 * PS], Ll[128 * PS];
  __shared__ int tok[PT];
  const int tid = threadIdx.x;
  const int col0 = blockIdx.x * PT;
  if (tid < PT) {
    const int c = col0 + tid;
    // last segment whose first column is <= c
    int lo = 0, hi = nseg;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (vstart(cu, mid) <= c) lo = mid; else hi = mid;
    }
    const int j = c - vstart(cu, lo);
    tok[tid] = (j >= 0 && j < cu[lo + 1] - cu[lo]) ? cu[lo] + j : -1;
  }
  __syncthreads();
  const int c4 = (tid & 31) * 4, r0 = tid >> 5;   // 4 features, 8 token rows per pass
  for (int half = 0; half < d_model; half += 128) {
    if (half) __syncthreads();
#pragma unroll 2
    for (int it = 0; it < PT / 8; ++it) {
      const int r = it * 8 + r0;
      const int t = tok[r];
      const int f = half + c4;
      float4 vq = make_float4(0.f, 0.f, 0.f, 0.f), vk = vq, vv = vq;
      if (t >= 0) {
        vq = *reinterpret_cast<const float4*>(q + (size_t)t * q_stride + f);
        vk = *reinterpret_cast<const float4*>(k + (size_t)t * k_stride + f);
        vv = *reinterpret_cast<const float4*>(v + (size_t)t * v_stride + f);
      }
      unsigned int ha, hb, la, lb;
      if (t >= 0) {
        split_pk_s(vq.x, vq.y, qmul, ha, la);
        split_pk_s(vq.z, vq.w, qmul, hb, lb);
        // Q / K planes are head-major [head][token][32]: a 64-key tile of one head
        // is 4 KiB contiguous (full 128-byte lines for the attention kernel's loads)
        const size_t hm = ((size_t)(f / HD) * t_total + t) * HD + f % HD;
        *reinterpret_cast<u32x2*>(qh + hm) = (u32x2){ha, hb};
        *reinterpret_cast<u32x2*>(ql + hm) = (u32x2){la, lb};
        split_pk_s(vk.x, vk.y, kmul, ha, la);
        split_pk_s(vk.z, vk.w, kmul, hb, lb);
        *reinterpret_cast<u32x2*>(kh + hm) = (u32x2){ha, hb};
        *reinterpret_cast<u32x2*>(kl + hm) = (u32x2){la, lb};
      }
      split_pk_s(vv.x, vv.y, vmul, ha, la);
      split_pk_s(vv.z, vv.w, vmul, hb, lb);
      const f16x4 vh4 = __builtin_bit_cast(f16x4, (u32x2){ha, hb});
      const f16x4 vl4 = __builtin_bit_cast(f16x4, (u32x2){la, lb});
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        Lh[(c4 + e) * PS + r] = vh4[e];
        Ll[(c4 + e) * PS + r] = vl4[e];
      }
    }
    __syncthreads();
    const int ch = (tid & 7) * 8, d0 = tid >> 3;   // 16-byte chunk, 32 feature rows per pass
    // plane order inside a 16-column group: [0-3, 8-11, 4-7, 12-15] (attn_vperm): the chunk at plane columns ch .. ch + 7
    // holds the tile columns c0 .. c0 + 3 and c0 + 8 .. c0 + 11, c0 = 16 (ch / 16) + 4 * ((ch / 8) & 1)
    const int c0 = (ch & ~15) + ((ch & 8) >> 1);
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int d = it * 32 + d0;
      if (half + d < d_model) {
        const u32x2 a0 = *reinterpret_cast<const u32x2*>(Lh + d * PS + c0), a1 = *reinterpret_cast<const u32x2*>(Lh + d * PS + c0 + 8);
        const u32x2 b0 = *reinterpret_cast<const u32x2*>(Ll + d * PS + c0), b1 = *reinterpret_cast<const u32x2*>(Ll + d * PS + c0 + 8);
        *reinterpret_cast<u32x4*>(vth + attn_v_off(half + d, col0 + ch, d_model)) = (u32x4){a0[0], a0[1], a1[0], a1[1]};
        *reinterpret_cast<u32x4*>(vtl + attn_v_off(half + d, col0 + ch, d_model)) = (u32x4){b0[0], b0[1], b1[0], b1[1]};
      }
    }
  }
}

// max over the two half-waves (lanes l and l^32) without touching LDS
__device__ __forceinline__ float half_swap_max(float x) {
  const unsigned int u = __float_as_uint(x);
  const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}

// ---------------------------------------------------------------------------------------------------
// The split-fp16 core ("s" = sum-checked): 32 queries per wave, 128 per workgroup.  Two choices take vector
// instructions off the per-score path (the kernel is bound by vector-instruction issue: profiles/r04_attn_counters.txt):
//  * no row-maximum pass in the steady state.  The lazy reference is set from the true maximum on the first tile;
//    afterwards a tile is exponentiated optimistically and the row sums the softmax needs anyway are the check: a
//    lane's 32 probabilities of the tile are all below their sum, so "sum < 2^15" proves that nothing left fp16's
//    range.  Otherwise (rare: a score more than ~10 octaves above the reference) the tile is recomputed after
//    recentring on its true maximum -- the loop below runs its body a second time, nothing of the tile has been
//    accumulated yet.  24 v_max + swap + compare per tile become one add and one compare.
//  * PLO = false ("single probability plane", attention mode 3): P is carried as ONE fp16 plane (round toward
//    zero) instead of hi + lo, O^T = (V_hi + V_lo)^T P_hi: 8 instead of 12 MFMAs for the second product and no
//    v_fma_mix pair per probability.  The row sum is formed from the ROUNDED plane (one v_fma_mix_f32 per half), so
//    numerator and denominator use the same weights: the output is an exact convex combination of the value rows
//    with weights perturbed by < 2^-10 relative each; the systematic part of the rounding cancels in 1 / l, what is
//    left is sum_j w_j delta_j (v_j - o), delta uniform over one fp16 ulp.
//    Q K^T keeps the three-product split in every H3 mode: score errors are amplified by the exponential.
// s_setprio 2 around the score MFMAs (-1.5 % in every mode).
// ADAPT (attention mode 4, needs H3 && PLO): the lo plane of the probabilities only where it matters.  A tile is
// "significant" for a wave when some lane holds a probability of at least sig_thr = 2^-5 (kAttnSigThr) of that lane's
// running row sum (the maximum of the tile's hi plane: 15 v_pk_max_f16); only such tiles pay for the lo plane (32
// quarter-rate v_fma_mix*_f16), the f32 sums and the third MFMA of every k-step.  The other tiles run as mode 3 (row
// sum from the rounded plane).  Every key with weight w_j >= 2^-5 is then carried with full accuracy; what the rest
// can contribute is bounded by 2^-10 sqrt(sum w_j^2) <= 2^-10 sqrt(2^-5) = 1.7e-4 of the value spread in the worst
// case (32 keys of exactly that weight) and is ~5e-6 for flat rows of 2 000 keys -- the peaked rows mode 3 is
// inaccurate on (few keys with large weights) are exact here.
// The key loop carries no tile bookkeeping in vector registers ("the key loop"): a tile's
// position is in the scalar base of its four DMA instructions, the LDS destinations are scalars, full tiles never
// clamp a row (only the fetch of the tail tile does), and the loop is unrolled by two so that the buffer index is
// static and every fragment read is a loop-invariant lane base plus an immediate offset.  Mode 4, a tile with two
// non-significant halves: 110 vector instructions for 20 MFMAs (was 142).
// A wave whose 32 queries all lie past the cloud's end runs the same loop WITHOUT the tile work (a second instance of
// the loop, not a branch inside it: a branch around the tile body moves the compiler's waits for the staged tiles
// into the loop); it writes nothing, except zeros for its 32 padding rows of the tiled output.
template <bool H3, bool PLO, int WPS, bool ADAPT = false>
__global__ __launch_bounds__(256, WPS) void k_attn_s(
    const _Float16* __restrict__ qh_g, const _Float16* __restrict__ ql_g,
    const _Float16* __restrict__ kh_g, const _Float16* __restrict__ kl_g,
    const _Float16* __restrict__ vth_g, const _Float16* __restrict__ vtl_g, int t_total, int tp,
    const int* __restrict__ cu, const int* __restrict__ kv_seg, int nseg, int nhead,
    const float* __restrict__ scales, float* __restrict__ out, int o_stride, float* __restrict__ lse_out,
    const int* __restrict__ o_tiles, float sig_thr) {
  static_assert(H3 || !PLO, "a lo plane of P only with split operands");
  static_assert(!ADAPT || (H3 && PLO), "the adaptive form is a refinement of the split form");
  // K tiles arrive by LDS-DMA (global_load_lds_dwordx4: no staging registers, no ds_write): the image is lane-linear,
  // 64 key rows of 64 bytes; the 16-byte chunk c of row r sits at position c ^ ((r >> 2) & 3) (the DMA lane fetches the
  // SOURCE chunk of its position: linear destination + swizzled source + the same XOR on the read), which makes the
  // fragment reads (16 lanes = 16 rows, one chunk) conflict-free without row padding.
  // V^T tiles the same way: 32 feature rows of 128 bytes (64 keys in the planes' fragment order, attn_vperm); chunk c of
  // row d at position c ^ ((d >> 1) & 7).
  // ONE LDS object for all planes: a lane's fragment reads of the hi and lo plane and of both buffers then share a base
  // register and differ in the instruction's immediate offset only.
  __shared__ __align__(16) _Float16 lds[H3 ? 4 : 2][2][KT2 * HD];   // [Kh, Vth, Kl, Vtl][buffer][tile image]
  _Float16(*const Kh)[KT2 * HD] = lds[0], (*const Vth)[KT2 * HD] = lds[1];
  _Float16(*const Kl)[KT2 * HD] = lds[H3 ? 2 : 0], (*const Vtl)[KT2 * HD] = lds[H3 ? 3 : 1];   // (!H3: never used)
  int seg, head, qt;
  {
    const int nqt = gridDim.x / (nhead * nseg);
    const int ngrp = nhead * nseg;
    const int b = blockIdx.x;
    if ((ngrp & 7) == 0) {      // all query tiles of one (segment, head) on one XCD (ids b and b + 8 share an L2)
      const int xcd = b & 7, idx = b >> 3;
      const int g = xcd + 8 * (idx / nqt);
      qt = idx % nqt;
      head = g % nhead;
      seg = g / nhead;
    } else {
      qt = b % nqt;
      head = (b / nqt) % nhead;
      seg = b / (nqt * nhead);
    }
  }
  const int qbeg = cu[seg], qlen = cu[seg + 1] - qbeg;
  const int q0 = qt * 128;
  if (q0 >= qlen) return;
  const int ks = kv_seg[seg];
  const int kbeg = cu[ks], klen = cu[ks + 1] - kbeg;
  const int vbeg = vstart(cu, ks);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // a scalar: LDS-DMA destinations, the empty-wave branch
  const int l31 = lane & 31, lh = lane >> 5;
  const int hoff = head * HD;
  // A wave whose 32 queries all lie past the cloud's end (the workgroup itself has q0 < qlen) takes its part in every
  // K / V^T DMA, wait and barrier -- the other waves' tiles depend on them -- and nothing else: no Q loads, no tile().
  const bool has_q = q0 + wave * 32 < qlen;

  f16x8 qh[2] = {}, ql[2] = {};
  if (has_q) {
    const int qi = min(q0 + wave * 32 + l31, qlen - 1);
    const size_t row = ((size_t)head * t_total + qbeg + qi) * HD + 8 * lh;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      qh[s] = *reinterpret_cast<const f16x8*>(qh_g + row + 16 * s);
      if constexpr (H3) ql[s] = *reinterpret_cast<const f16x8*>(ql_g + row + 16 * s);
    }
  }
  // The Q fragments are first USED inside the tile loop: without this the compiler's own wait for their loads
  // lands in the loop (s_waitcnt vmcnt(0) in front of the score MFMAs) and drains the asm-issued prefetch of the
  // next K / V tile on every iteration.
  if constexpr (H3) asm volatile("" ::"v"(qh[0]), "v"(qh[1]), "v"(ql[0]), "v"(ql[1]));
  else asm volatile("" ::"v"(qh[0]), "v"(qh[1]));
  f32x16 o, negm;      // negm: all registers = off - m_ref, the C operand of the score MFMAs
  float psum = 0.f;    // per-lane partial row sum (the two half-waves are joined at the end)
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    o[r] = 0.f;
    negm[r] = 0.f;
  }

  const int skr = tid >> 2, skc = ((tid & 3) ^ ((tid >> 4) & 3)) * 8;   // K: row, SOURCE chunk of this lane's position
  const int svr = tid >> 3, svc = ((tid & 7) ^ ((tid >> 4) & 7)) * 8;   // V^T: row, SOURCE chunk of this lane's position
  // No address arithmetic per tile in vector registers: a tile's position goes into the SCALAR base of the DMA (K planes:
  // 64 rows of 64 bytes per tile; blocked V^T planes: four 16-column blocks, vbeg is 16-aligned and kt a multiple of
  // 64), the lane's offset inside a tile is the same for every tile, and the four LDS destinations are scalars (wave).
  // Only the fetch of a TAIL tile (kt + 64 > klen) clamps its K rows to the segment's last key.
  const unsigned kdst_h = (unsigned)(uintptr_t)(&Kh[0][0]) + (unsigned)wave * 1024u;   // + buf * 4096
  const unsigned kdst_l = (unsigned)(uintptr_t)(&Kl[0][0]) + (unsigned)wave * 1024u;
  const unsigned vdst_h = (unsigned)(uintptr_t)(&Vth[0][0]) + (unsigned)wave * 1024u;
  const unsigned vdst_l = (unsigned)(uintptr_t)(&Vtl[0][0]) + (unsigned)wave * 1024u;
  const size_t kbase = ((size_t)head * t_total + kbeg) * HD;                                   // halves, tile 0
  const size_t vbase = attn_v_off(hoff, (size_t)vbeg, nhead * HD);
  const unsigned vstep = (unsigned)(nhead * HD * KT2);                                          // halves per tile
  const unsigned koff = (unsigned)(skr * HD + skc) * 2u;                                        // bytes inside a tile
  const unsigned voff = (unsigned)attn_v_off(svr, (size_t)svc, nhead * HD) * 2u;
  auto fetch = [&](int kt, int nbuf, auto tail_tag) __attribute__((always_inline)) {   // nbuf: the buffer tile kt will be read from
    const size_t kel = kbase + (size_t)(unsigned)kt * HD, vel = vbase + (size_t)((unsigned)kt / KT2) * vstep;
    const _Float16 *kh_t = kh_g + kel, *kl_t = kl_g + kel, *vth_t = vth_g + vel, *vtl_t = vtl_g + vel;
    const unsigned ko = decltype(tail_tag)::value ? (unsigned)(min(skr, klen - 1 - kt) * HD + skc) * 2u : koff;
    lds_dma16_first(kh_t, ko, kdst_h + (unsigned)nbuf * 4096u);
    if constexpr (H3) lds_dma16_first(kl_t, ko, kdst_l + (unsigned)nbuf * 4096u);
    lds_dma16_first(vth_t, voff, vdst_h + (unsigned)nbuf * 4096u);
    if constexpr (H3) lds_dma16_first(vtl_t, voff, vdst_l + (unsigned)nbuf * 4096u);
  };
  // the fetch of the tile at kt, if there is one: full tiles never clamp
  auto fetch_next = [&](int kt, int nbuf) __attribute__((always_inline)) {
    if (kt + KT2 <= klen) fetch(kt, nbuf, std::false_type{});
    else if (kt < klen) fetch(kt, nbuf, std::true_type{});
  };
  auto stash = [&]() {
    wait_vm<0>();      // this wave's pieces of the next tile have landed
  };

  constexpr float kOff = 4.0f;        // a fresh reference puts the row maximum at 2^kOff
  constexpr float kSumMax = 32768.f;  // a lane's tile sum below this: every probability inside fp16's range
  const float kSig = sig_thr;         // ADAPT: a probability below kSig x the lane's running sum needs no lo plane

  // buf: an integral_constant in the steady state (LDS reads at immediate offsets); l31, lh: the lane's query and half
  auto tile = [&](int kt, auto buf, auto tail_tag, int l31, int lh) {
    constexpr bool TAIL = decltype(tail_tag)::value;
    f32x16 sc[2];
    unsigned int ph_u[2][8], pl_u[2][8];
    float ts = 0.f;
    bool redo = false;
    bool sigk[2] = {PLO, PLO};      // does the 32-key sub-tile carry a lo plane (ADAPT: decided per sub-tile)
    for (;;) {
      // ---- S^T = K Q^T + (off - m_ref)   (rows = keys, cols = queries) ----
      __builtin_amdgcn_s_setprio(2);
      f16x8 kfh[2][2], kfl[2][2];
      auto load_kf = [&](int kk) __attribute__((always_inline)) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const int kpos = (32 * kk + l31) * HD + 8 * ((2 * s + lh) ^ ((l31 >> 2) & 3));
          kfh[kk][s] = *reinterpret_cast<const f16x8*>(Kh[buf] + kpos);
          if constexpr (H3) kfl[kk][s] = *reinterpret_cast<const f16x8*>(Kl[buf] + kpos);
        }
      };
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        load_kf(kk);
        sc[kk] = negm;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          if constexpr (H3) sc[kk] = mma3_32(kfh[kk][s], kfl[kk][s], qh[s], ql[s], sc[kk]);
          else sc[kk] = mma1_32(kfh[kk][s], qh[s], sc[kk]);
        }
        if (kk == 0) __builtin_amdgcn_sched_barrier(0);
      }
      __builtin_amdgcn_s_setprio(0);
      if (TAIL) {
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int j = acc_row32(r, lh, kt + 32 * kk);
            if (j >= klen) sc[kk][r] = -INFINITY;
          }
      }
      const bool first = kt == 0;
      if (first || redo) {
        // recentre on the tile's true maximum (first tile: o and psum are still zero)
        float mx = fmaxf(sc[0][0], sc[1][0]);
#pragma unroll
        for (int r = 1; r < 16; ++r) mx = fmaxf(mx, fmaxf(sc[0][r], sc[1][r]));
        mx = half_swap_max(mx);
        const float delta = first ? mx - kOff : fmaxf(mx - kOff, 0.f);
        const float corr = first ? 1.0f : __builtin_amdgcn_exp2f(-delta);
        psum *= corr;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          o[r] *= corr;
          negm[r] -= delta;
          sc[0][r] -= delta;
          sc[1][r] -= delta;
        }
      }
      // ---- probabilities, their planes and the lane's tile sum ----
      float ta = 0.f, tb = 0.f;
      if constexpr (ADAPT) {
        // per 32-key sub-tile (the decision needs that sub-tile's probabilities only: 16 live registers, not 32)
        const float thr = kSig * psum;                                    // (first tile: psum = 0 -> significant)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          f16x2 m2 = {(_Float16)0.f, (_Float16)0.f};
#pragma unroll
          for (int r = 0; r < 16; r += 2) {
            const float p0 = __builtin_amdgcn_exp2f(sc[kk][r]);
            const float p1 = __builtin_amdgcn_exp2f(sc[kk][r + 1]);
            sc[kk][r] = p0;
            sc[kk][r + 1] = p1;
            // round to NEAREST here (v_cvt_pk_f16_f32, gfx950): sub-tiles with and without a lo plane are mixed in
            // one row, so the systematic part of a round-toward-zero plane (-2^-11.5 on average) would no longer
            // cancel in 1 / l as it does when EVERY weight carries it (mode 3) -- measured 4e-5 of the output scale
            // on the late-spike test before this
            // (through the compiler, not inline asm: a VALU instruction that reads the result of a transcendental needs
            // a wait state the hazard pass only inserts for instructions it can see -- the asm form produced NaNs in
            // the lanes the quarter-rate unit finishes last)
            const unsigned int hi_u = __builtin_bit_cast(unsigned int, __builtin_convertvector((f32x2){p0, p1}, f16x2));
            ph_u[kk][r >> 1] = hi_u;
            m2 = __builtin_elementwise_max(m2, __builtin_bit_cast(f16x2, hi_u));
          }
          const float mxp = (float)(m2[0] > m2[1] ? m2[0] : m2[1]);
          sigk[kk] = __builtin_amdgcn_ballot_w64(!(mxp < thr)) != 0;
          if (sigk[kk]) {
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
              ta += sc[kk][r];
              tb += sc[kk][r + 1];
              unsigned int lo_u;
              asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]\n\t"
                  "v_fma_mixhi_f16 %0, %1, -1.0, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]"
                  : "=&v"(lo_u)
                  : "v"(ph_u[kk][r >> 1]), "v"(sc[kk][r]), "v"(sc[kk][r + 1]));
              pl_u[kk][r >> 1] = lo_u;
            }
          } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
              asm("v_fma_mix_f32 %0, %1, 1.0, %0 op_sel_hi:[1,0,0]" : "+v"(ta) : "v"(ph_u[kk][i]));
              asm("v_fma_mix_f32 %0, %1, 1.0, %0 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(tb) : "v"(ph_u[kk][i]));
            }
          }
        }
      } else {
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
          const float p0 = __builtin_amdgcn_exp2f(sc[kk][r]);
          const float p1 = __builtin_amdgcn_exp2f(sc[kk][r + 1]);
          const auto hi_h = __builtin_amdgcn_cvt_pkrtz(p0, p1);
          const unsigned int hi_u = __builtin_bit_cast(unsigned int, hi_h);
          ph_u[kk][r >> 1] = hi_u;
          if constexpr (PLO) {
            ta += p0;      // two plain adds (-fno-slp-vectorize): v_pk_add_f32 issues slower than the pair
            tb += p1;
            unsigned int lo_u;
            asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]\n\t"
                "v_fma_mixhi_f16 %0, %1, -1.0, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]"
                : "=&v"(lo_u)
                : "v"(hi_u), "v"(p0), "v"(p1));
            pl_u[kk][r >> 1] = lo_u;
          } else {
            // the sum of the ROUNDED pair: acc += float(half) exactly, one v_fma_mix_f32 per half (a v_dot2c_f32_f16
            // per pair costs 2.7 ns beside an MFMA, these 0.4 each: scripts/abl/issue_probe.hip, round 5)
            asm("v_fma_mix_f32 %0, %1, 1.0, %0 op_sel_hi:[1,0,0]" : "+v"(ta) : "v"(hi_u));
            asm("v_fma_mix_f32 %0, %1, 1.0, %0 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(tb) : "v"(hi_u));
          }
        }
      }
      ts = ta + tb;
      if (redo || __builtin_amdgcn_ballot_w64(!(ts < kSumMax)) == 0) break;
      redo = true;   // some probability may have left fp16's range: once more, recentred (rare)
    }
    psum += ts;
    // ---- O^T += V^T P^T ----
    auto pv = [&](auto lo_tag, int kk) __attribute__((always_inline)) {
      constexpr bool LO = decltype(lo_tag)::value;
      f16x8 vfh[2], vfl[2];
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int vpos = l31 * KT2 + 8 * ((4 * kk + 2 * s + lh) ^ ((l31 >> 1) & 7));
        vfh[s] = *reinterpret_cast<const f16x8*>(Vth[buf] + vpos);
        if constexpr (H3) vfl[s] = *reinterpret_cast<const f16x8*>(Vtl[buf] + vpos);
      }
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const u32x4 pa = {ph_u[kk][4 * s], ph_u[kk][4 * s + 1], ph_u[kk][4 * s + 2], ph_u[kk][4 * s + 3]};
        const f16x8 pbh = __builtin_bit_cast(f16x8, pa);
        if constexpr (LO) {
          const u32x4 pb = {pl_u[kk][4 * s], pl_u[kk][4 * s + 1], pl_u[kk][4 * s + 2], pl_u[kk][4 * s + 3]};
          const f16x8 pbl = __builtin_bit_cast(f16x8, pb);
          o = mma1_32(vfh[s], pbl, o);
        }
        if constexpr (H3) o = mma1_32(vfl[s], pbh, o);
        o = mma1_32(vfh[s], pbh, o);
      }
    };
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      if (kk == 1) __builtin_amdgcn_sched_barrier(0);
      if constexpr (ADAPT) {
        if (sigk[kk]) pv(std::true_type{}, kk);
        else pv(std::false_type{}, kk);
      } else {
        pv(std::integral_constant<bool, PLO>{}, kk);
      }
    }
  };

  // The key loop, unrolled by two so that the buffer index is a compile-time constant in the steady state: step(B) runs
  // the full tile at kt out of buffer B while the DMA brings the next tile into buffer B ^ 1.  One barrier per tile: at
  // the end of a step every wave has finished reading buffer B and has seen its own pieces of the next tile land.
  auto key_loop = [&](auto work_tag) __attribute__((always_inline)) {
    constexpr bool WORK = decltype(work_tag)::value;
    int kt = 0;
    fetch_next(0, 0);
    stash();
    __syncthreads();
    auto step = [&](auto buf_tag) __attribute__((always_inline)) {
      constexpr int B = decltype(buf_tag)::value;
      if (kt + KT2 > klen) return false;
      fetch_next(kt + KT2, B ^ 1);
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (WORK) tile(kt, buf_tag, std::false_type{}, l31, lh);
      __builtin_amdgcn_sched_barrier(0);
      stash();
      __syncthreads();
      kt += KT2;
      return true;
    };
    int buf = 0;
    for (;;) {
      if (!step(std::integral_constant<int, 0>{})) break;
      buf = 1;
      if (!step(std::integral_constant<int, 1>{})) break;
      buf = 0;
    }
    if constexpr (WORK) {
      if (kt < klen) {
        // The tail tile reads its buffer through a run-time index.  Its lane id is opaque: the LDS read positions are
        // formed again here, once -- otherwise the compiler forms a second set in front of the loop and spills it.
        int tl = lane;
        asm volatile("" : "+v"(tl));
        tile(kt, buf, std::true_type{}, tl & 31, tl >> 5);
      }
    }
  };
  if (has_q) key_loop(std::true_type{});
  else key_loop(std::false_type{});

  if (!has_q) {
    // tiled output (below): zeros for the wave's 32 padding rows -- finite, the chains compute on them and drop them
    if (o_tiles != nullptr) {
      float4* op = reinterpret_cast<float4*>(out) + ((size_t)(o_tiles[seg] + qt) * 4 + wave) * 2048 + lane;
#pragma unroll
      for (int g = 0; g < 4; ++g) op[(4 * head + g) * 64] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    return;
  }
  float l_run = psum;
  l_run += __shfl_xor(l_run, 32, 64);
  const int qi = q0 + wave * 32 + l31;
  // log2 sum_j 2^(s_ij): handed to the backward (training)
  if (lse_out != nullptr && qi < qlen && lh == 0)
    lse_out[(size_t)(qbeg + qi) * nhead + head] = __builtin_amdgcn_logf(l_run) - negm[0];
  if (o_tiles != nullptr) {
    // Tiled output for the fused row chains (xenc.hip, "tiled token tensors"): this workgroup's 128 queries are chain tile
    // o_tiles[seg] + qt, the wave's 32 queries one 32 KiB wave block of it, and the lane's four features 8 g + 4 lh .. + 3
    // of head `head` are the 16-byte piece (4 head + g, lane) of that block -- what the chain's lane (token l31, half lh)
    // loads with ONE coalesced instruction per piece.  Every lane stores (rows past the cloud's end hold the clamped last
    // query's finite values: the chain computes on them and drops them).
    const float inv = (l_run > 0.f ? 1.0f / l_run : 0.f) * scales[3];
    float4* op = reinterpret_cast<float4*>(out) + ((size_t)(o_tiles[seg] + qt) * 4 + wave) * 2048 + lane;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float4 w4;
      w4.x = o[4 * g + 0] * inv;
      w4.y = o[4 * g + 1] * inv;
      w4.z = o[4 * g + 2] * inv;
      w4.w = o[4 * g + 3] * inv;
      op[(4 * head + g) * 64] = w4;
    }
  } else if (qi < qlen) {
    const float inv = (l_run > 0.f ? 1.0f / l_run : 0.f) * scales[3];   // 2^-ev undoes the V multiplier
    float* op = out + (size_t)(qbeg + qi) * o_stride + hoff;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float4 w4;
      w4.x = o[4 * g + 0] * inv;
      w4.y = o[4 * g + 1] * inv;
      w4.z = o[4 * g + 2] * inv;
      w4.w = o[4 * g + 3] * inv;
      *reinterpret_cast<float4*>(op + 8 * g + 4 * lh) = w4;
    }
  }
}

static std::atomic<int> g_attn_mode{4};   // 4 = adaptive lo plane (default), 1 = split-fp16, 0 = exact f32 MFMA, 2 = single-pass fp16,
                                          // 3 = split-fp16 scores, ONE probability plane (k_attn_s<true, false>), 4 = adaptive lo plane

// L1 norm of every row of w [rows, cols]: one wave per row.
__global__ void k_row_l1(const float* __restrict__ w, int rows, int cols, float* __restrict__ out) {
  const int row = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  float s = 0.f;
  for (int c = lane; c < cols; c += 64) s += fabsf(w[(size_t)row * cols + c]);
  s = wave_sum(s);
  if (lane == 0) out[row] = s;
}

// Plane multipliers from bounds on |q|, |k|, |v| (one workgroup).
//   rowl1 == nullptr: the bounds are the measured maxima (q_parts, k_parts, v_parts);
//   else (fused in-projection, weights [3d, d], bias [3d]): bound of block b =
//     max|x| * max_row L1(W_b) + max|bias_b|, x = x_qk for Q and K, x_v for V.
__global__ __launch_bounds__(256) void k_plane_scales(const float* __restrict__ q_parts,
                                                      const float* __restrict__ k_parts,
                                                      const float* __restrict__ v_parts,
                                                      const float* __restrict__ rowl1,
                                                      const float* __restrict__ bias, int d, float qscale,
                                                      float* __restrict__ scales, int nq_parts, int nk_parts,
                                                      int nv_parts, float* __restrict__ out_range) {
  __shared__ float sh[17];
  __shared__ float blk[6];
  float qb = block_absmax(q_parts, sh, nq_parts);
  float kb = k_parts == q_parts ? qb : block_absmax(k_parts, sh, nk_parts);   // shared input: reduce once
  float vb = v_parts == q_parts ? qb : block_absmax(v_parts, sh, nv_parts);
  if (rowl1 != nullptr) {
    for (int b = 0; b < 3; ++b) {
      float l1 = 0.f, bm = 0.f;
      for (int i = threadIdx.x; i < d; i += 256) {
        l1 = fmaxf(l1, rowl1[b * d + i]);
        bm = fmaxf(bm, fabsf(bias[b * d + i]));
      }
      l1 = wave_max(l1);
      bm = wave_max(bm);
      __syncthreads();
      if ((threadIdx.x & 63) == 0) {
        sh[threadIdx.x >> 6] = l1;
        sh[4 + (threadIdx.x >> 6)] = bm;
      }
      __syncthreads();
      if (threadIdx.x == 0) {
        blk[2 * b] = fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
        blk[2 * b + 1] = fmaxf(fmaxf(sh[4], sh[5]), fmaxf(sh[6], sh[7]));
      }
    }
    __syncthreads();
    qb = qb * blk[0] + blk[1];
    kb = kb * blk[2] + blk[3];
    vb = vb * blk[4] + blk[5];
  }
  if (threadIdx.x == 0) {
    // ek = half the exponent gap: K 2^ek and Q qscale 2^-ek both sit at sqrt(|q||k|)
    const float qs = qb * qscale;
    int ek = 0;
    if (qs > 0.f && kb > 0.f && qs < 3.0e38f && kb < 3.0e38f) {
      const int eq = (int)((__float_as_uint(qs) >> 23) & 0xff) - 127;
      const int ekk = (int)((__float_as_uint(kb) >> 23) & 0xff) - 127;
      ek = (eq - ekk) >> 1;
      ek = max(-60, min(60, ek));
    }
    const int ev = pow2_exp_for(vb);
    scales[0] = qscale * pow2f(-ek);
    scales[1] = pow2f(ek);
    scales[2] = pow2f(ev);
    scales[3] = pow2f(-ev);
    // the attention output is a convex combination of value rows: |out| <= max |v| < 2^(15 - ev)
    if (out_range) out_range[0] = pow2f(15 - ev);
  }
}

}  // namespace
}  // namespace spr

using namespace spr;

static size_t attn_tp_(int t, int nseg) { return align_up((size_t)t + 16 * (size_t)nseg + KT2, PT); }

namespace {
// small scratch behind the planes: 3 absmax partial arrays, the row norms of the in-projection's weights, 4 scales
struct AttnSmall {
  float *p0, *p1, *p2, *rowl1, *scales;
};
// The operand planes and the small scratch; t = 0 is measured as one token (the size queries' clamp).
void attn_layout(Workspace& w, int t, int nseg, size_t d, AttnPlanes& pl, AttnSmall& sm) {
  const size_t T = (size_t)(t > 0 ? t : 1), tp = attn_tp_(t, nseg);
  pl.qh = w.take<_Float16>(T * d);
  pl.ql = w.take<_Float16>(T * d);
  pl.kh = w.take<_Float16>(T * d);
  pl.kl = w.take<_Float16>(T * d);
  pl.vth = w.take<_Float16>(d * tp);
  pl.vtl = w.take<_Float16>(d * tp);
  sm.p0 = w.take<float>(kAmaxParts);
  sm.p1 = w.take<float>(kAmaxParts);
  sm.p2 = w.take<float>(kAmaxParts);
  sm.rowl1 = w.take<float>(1024);
  pl.scales = sm.scales = w.take<float>(4);
}
// spr_attn_inproj_varlen_fwd: the same, then (exact mode and tiny inputs only) the fp32 [t, 3 d] projection
struct InprojWs {
  size_t planes_bytes;   // what attn_layout took: the unfused core carves the same bytes again
  float* qkv;
};
InprojWs attn_inproj_layout(Workspace& w, int t, int nseg, size_t d, AttnPlanes& pl, AttnSmall& sm) {
  attn_layout(w, t, nseg, d, pl, sm);
  InprojWs l;
  l.planes_bytes = w.off;
  l.qkv = w.take<float>((size_t)(t > 0 ? t : 1) * 3 * d);
  return l;
}
}  // namespace

extern "C" size_t spr_attn_workspace_bytes(int t, int nseg, int nhead, int head_dim) {
  if (t < 0 || nseg < 0 || nhead < 0 || head_dim < 0) return 0;
  Workspace w;
  AttnPlanes pl{};
  AttnSmall sm{};
  attn_layout(w, t, nseg, (size_t)nhead * head_dim, pl, sm);
  return w.used();
}

namespace {
// does the core launched for `mode` write the per-query log-sum-exp (lse_out)?  k_attn_s does, k_attn does not.
bool attn_core_writes_lse(int mode) { return mode != 0; }

// attention mode 4: a tile needs the lo plane of its probabilities when one of them reaches this share of the lane's
// running row sum (k_attn_s, ADAPT)
constexpr float kAttnSigThr = 0x1p-5f;

// modes 1 .. 4: the sum-checked core k_attn_s, one instantiation per mode.  Three waves per SIMD (168-register
// budget); mode 4 four.
int launch_core(const AttnPlanes& pl, int t, size_t tp, const int* cu, const int* kv_seg, int nseg,
                int max_len_host, int nhead, float* out, int o_stride, int mode, hipStream_t stream,
                float* lse_out = nullptr, const int* o_tiles = nullptr) {
  ProfScope prof(stream, -1, t);
  dim3 grid(cdiv(max_len_host, QB) * nhead * nseg);
#define SPR_ATTN_S(H3_, PLO_, WPS_, ADAPT_)                                                                          \
  hipLaunchKernelGGL((k_attn_s<H3_, PLO_, WPS_, ADAPT_>), grid, dim3(256), 0, stream, pl.qh, pl.ql, pl.kh, pl.kl,   \
                     pl.vth, pl.vtl, t, (int)tp, cu, kv_seg, nseg, nhead, pl.scales, out, o_stride, lse_out, o_tiles, \
                     kAttnSigThr)
  if (mode == 4) SPR_ATTN_S(true, true, 4, true);
  else if (mode == 3) SPR_ATTN_S(true, false, 3, false);
  else if (mode == 2) SPR_ATTN_S(false, false, 3, false);
  else SPR_ATTN_S(true, true, 3, false);
#undef SPR_ATTN_S
  SPR_LAUNCH_CHECK();
  return 0;
}
}  // namespace

// lse (NULL = not wanted): receives [t, nhead] = log2 sum_j 2^(log2(e) q_i.k_j scale) per query and head for
// spr_attn_varlen_bwd (the backward then skips its own pass over the keys).  *lse_written = 0 in
// exact-f32 mode (attention mode 0, whose core does not produce it): lse is then untouched.
extern "C" int spr_attn_varlen_fwd(const float* q, int q_stride, const float* k, int k_stride, const float* v,
                                   int v_stride, const int* cu, const int* kv_seg, int t, int nseg,
                                   int max_len_host, int nhead, int head_dim, float scale, float* out, int o_stride,
                                   float* lse, int* lse_written, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPR_REQUIRE(lse == nullptr || lse_written != nullptr, "attention: lse needs lse_written");
  SPR_REQUIRE(head_dim == HD, "attention: head_dim must be %d (got %d)", HD, head_dim);
  SPR_REQUIRE(t >= 1 && nseg >= 1 && nhead >= 1 && max_len_host >= 1, "attention: bad sizes");
  SPR_REQUIRE(q_stride % 4 == 0 && k_stride % 4 == 0 && v_stride % 4 == 0 && o_stride % 4 == 0,
              "attention: row strides must be multiples of 4 floats");
  SPR_REQUIRE((long)cdiv(max_len_host, QB) * nhead * nseg < (1l << 31), "attention: grid too large");
  const int mode = spr::g_attn_mode.load(std::memory_order_relaxed);
  float* lse_out = nullptr;
  if (lse != nullptr) {
    *lse_written = attn_core_writes_lse(mode) ? 1 : 0;
    if (*lse_written) lse_out = lse;
  }
  if (mode == 0) {
    dim3 grid(cdiv(max_len_host, QB) * nhead * nseg);
    hipLaunchKernelGGL(k_attn, grid, dim3(256), 0, stream, q, q_stride, k, k_stride, v, v_stride, cu,
                       kv_seg, nseg, nhead, scale, out, o_stride);
    SPR_LAUNCH_CHECK();
    return 0;
  }
  const int d_model = nhead * head_dim;
  const size_t tp = attn_tp_(t, nseg);
  SPR_REQUIRE(tp < (1ul << 31), "attention: too many tokens");
  Workspace w(ws, ws_bytes);
  AttnPlanes pl{};
  AttnSmall sm{};
  attn_layout(w, t, nseg, d_model, pl, sm);
  SPR_REQUIRE(ws != nullptr && w.ok(), "attention: workspace too small (%zu bytes given)", ws_bytes);
  if (int rc = launch_absmax2(q, t, d_model, q_stride, sm.p0, k, t, d_model, k_stride, sm.p1, stream)) return rc;
  if (int rc = launch_absmax(v, t, d_model, v_stride, sm.p2, stream)) return rc;
  hipLaunchKernelGGL(k_plane_scales, dim3(1), dim3(256), 0, stream, sm.p0, sm.p1, sm.p2, (const float*)nullptr,
                     (const float*)nullptr, d_model, scale * 1.4426950408889634f, sm.scales, kAmaxParts, kAmaxParts,
                     kAmaxParts, (float*)nullptr);
  hipLaunchKernelGGL(k_attn_pack, dim3((unsigned)(tp / PT)), dim3(256), 0, stream, q, q_stride, k, k_stride,
                     v, v_stride, cu, nseg, d_model, t, (int)tp, sm.scales, pl.qh, pl.ql, pl.kh, pl.kl,
                     pl.vth, pl.vtl);
  SPR_LAUNCH_CHECK();
  return launch_core(pl, t, tp, cu, kv_seg, nseg, max_len_host, nhead, out, o_stride, mode, stream, lse_out);
}

extern "C" size_t spr_attn_inproj_workspace_bytes(int t, int nseg, int nhead, int head_dim) {
  if (t < 0 || nseg < 0 || nhead < 0 || head_dim < 0) return 0;
  Workspace w;
  AttnPlanes pl{};
  AttnSmall sm{};
  attn_inproj_layout(w, t, nseg, (size_t)nhead * head_dim, pl, sm);
  return w.used();
}

// Weight-side inputs of the fused in-projection, measured once per weight version:
// out[0 .. spr_range_parts()) = max |w| partials, then 3 d row L1 norms of w_in [3d, d].
extern "C" int spr_attn_inproj_prepare(const float* w_in, int d, float* out, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPR_REQUIRE(w_in != nullptr && out != nullptr && d >= 1 && 3 * d <= 1024, "inproj_prepare: bad arguments");
  if (int rc = launch_absmax(w_in, 3 * d, d, d, out, stream)) return rc;
  hipLaunchKernelGGL(k_row_l1, dim3(cdiv((long)3 * d * 64, 256)), dim3(256), 0, stream, w_in, 3 * d, d, out + kAmaxParts);
  SPR_LAUNCH_CHECK();
  return 0;
}

extern "C" int spr_attn_inproj_varlen_fwd(const float* x_qk, const float* x_v, int t, const float* w_in,
                                          const float* b_in, const int* cu, const int* kv_seg, int nseg,
                                          int max_len_host, int nhead, int head_dim, float scale, float* out,
                                          int o_stride, const float* xqk_range, int xqk_range_n,
                                          const float* xv_range, int xv_range_n, float* out_range,
                                          const float* w_prep, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPR_REQUIRE(head_dim == HD, "attention: head_dim must be %d (got %d)", HD, head_dim);
  SPR_REQUIRE(nhead * head_dim == 256, "attention in-projection: d_model must be 256 (got %d)", nhead * head_dim);
  SPR_REQUIRE(t >= 1 && nseg >= 1 && max_len_host >= 1, "attention: bad sizes");
  SPR_REQUIRE(x_qk && x_v && w_in && b_in, "attention in-projection: null operand");
  const int d = nhead * head_dim;
  const int mode = spr::g_attn_mode.load(std::memory_order_relaxed);
  const size_t tp = attn_tp_(t, nseg);
  SPR_REQUIRE(tp < (1ul << 31), "attention: too many tokens");
  Workspace w(ws, ws_bytes);
  AttnPlanes pl{};
  AttnSmall sm{};
  const auto [planes_bytes, qkv] = attn_inproj_layout(w, t, nseg, d, pl, sm);
  SPR_REQUIRE(ws != nullptr && w.ok(), "attention in-projection: workspace too small (%zu bytes given)", ws_bytes);
  const bool gemm_split = gemm_mode() == 1;
  if (mode == 0 || t < 256 || !gemm_split) {
    if (out_range != nullptr) {   // this route publishes no range: an infinite bound would be wrong, so measure later
      SPR_REQUIRE(false, "attention in-projection: out_range is only available on the fused split-fp16 path "
                         "(attn mode %d, gemm split %d, t=%d)", mode, (int)gemm_split, t);
    }
    // exact-f32 mode (and tiny inputs): plain projection into the workspace, then the
    // unfused core -- same results as spr_linear + spr_attn_varlen_fwd
    const float *xp = nullptr, *xvp = nullptr, *wp = nullptr;
    if (gemm_split) {   // operand ranges for the split-fp16 GEMM (sm.* is rewritten by the core afterwards)
      if (int rc = launch_absmax(x_qk, t, d, d, sm.p0, stream)) return rc;
      if (int rc = launch_absmax(w_in, 3 * d, d, d, sm.p1, stream)) return rc;
      xp = xvp = sm.p0;
      wp = sm.p1;
      if (x_v != x_qk) {
        if (int rc = launch_absmax(x_v, t, d, d, sm.p2, stream)) return rc;
        xvp = sm.p2;
      }
    }
    if (x_v == x_qk) {
      if (int rc = launch_linear_ranged(x_qk, t, d, w_in, 3 * d, b_in, qkv, xp, wp, stream)) return rc;
    } else {
      // two projections, written side by side: [q | k] from x_qk, [v] from x_v
      float* qk = qkv;
      float* v = qkv + (size_t)t * 2 * d;
      if (int rc = launch_linear_ranged(x_qk, t, d, w_in, 2 * d, b_in, qk, xp, wp, stream)) return rc;
      if (int rc = launch_linear_ranged(x_v, t, d, w_in + (size_t)2 * d * d, d, b_in + 2 * d, v, xvp, wp, stream))
        return rc;
      return spr_attn_varlen_fwd(qk, 2 * d, qk + d, 2 * d, v, d, cu, kv_seg, t, nseg, max_len_host, nhead,
                                 head_dim, scale, out, o_stride, nullptr, nullptr, ws, planes_bytes, stream_);
    }
    return spr_attn_varlen_fwd(qkv, 3 * d, qkv + d, 3 * d, qkv + 2 * d, 3 * d, cu, kv_seg, t, nseg,
                               max_len_host, nhead, head_dim, scale, out, o_stride, nullptr, nullptr, ws, planes_bytes,
                               stream_);
  }
  SPR_REQUIRE((long)cdiv(max_len_host, QB) * nhead * nseg < (1l << 31), "attention: grid too large");
  pl.cu = cu;
  pl.nseg = nseg;
  pl.t_total = t;
  pl.tp = (int)tp;
  // operand ranges: max|x| (inputs), max|w| (the projection's own operand scale) and the plane
  // multipliers from the bounds max|x| * max row-L1(W block) + max|bias block|
  // input ranges: published by the producer (LayerNorm) or measured here
  // weight side (max |w| partials + row L1 norms): measured here, or once per weight version by
  // the caller (spr_attn_inproj_prepare -> w_prep)
  const float* wparts = w_prep != nullptr ? w_prep : sm.p1;
  const float* rowl1 = w_prep != nullptr ? w_prep + kAmaxParts : sm.rowl1;
  const float* xqp = sm.p0;
  int n_xq = kAmaxParts;
  if (xqk_range != nullptr) {
    SPR_REQUIRE(xqk_range_n >= 1, "attention in-projection: xqk_range needs a count");
    xqp = xqk_range;
    n_xq = xqk_range_n;
    if (w_prep == nullptr)
      if (int rc = launch_absmax(w_in, 3 * d, d, d, sm.p1, stream)) return rc;
  } else if (w_prep == nullptr) {
    if (int rc = launch_absmax2(x_qk, t, d, d, sm.p0, w_in, 3 * d, d, d, sm.p1, stream)) return rc;
  } else {
    if (int rc = launch_absmax(x_qk, t, d, d, sm.p0, stream)) return rc;
  }
  const float* xvp = xqp;
  int n_xv = n_xq;
  if (x_v != x_qk) {
    if (xv_range != nullptr) {
      SPR_REQUIRE(xv_range_n >= 1, "attention in-projection: xv_range needs a count");
      xvp = xv_range;
      n_xv = xv_range_n;
    } else {
      if (int rc = launch_absmax(x_v, t, d, d, sm.p2, stream)) return rc;
      xvp = sm.p2;
      n_xv = kAmaxParts;
    }
  }
  if (w_prep == nullptr)
    hipLaunchKernelGGL(k_row_l1, dim3(cdiv((long)3 * d * 64, 256)), dim3(256), 0, stream, w_in, 3 * d, d, sm.rowl1);
  hipLaunchKernelGGL(k_plane_scales, dim3(1), dim3(256), 0, stream, xqp, xqp, xvp, rowl1, b_in, d,
                     scale * 1.4426950408889634f, sm.scales, n_xq, n_xq, n_xv, out_range);
  hipLaunchKernelGGL(k_attn_zero_gaps, dim3(d), dim3(256), 0, stream, cu, nseg, (int)tp, pl.vth, pl.vtl);
  if (x_v == x_qk) {
    if (int rc = launch_inproj_planes(x_qk, t, d, w_in, 3 * d, b_in, 0, pl, xqp, n_xq, wparts, stream)) return rc;
  } else {
    if (int rc = launch_inproj_planes(x_qk, t, d, w_in, 2 * d, b_in, 0, pl, xqp, n_xq, wparts, stream)) return rc;
    if (int rc = launch_inproj_planes(x_v, t, d, w_in + (size_t)2 * d * d, d, b_in + 2 * d, 2 * d, pl, xvp, n_xv, wparts,
                                      stream))
      return rc;
  }
  return launch_core(pl, t, tp, cu, kv_seg, nseg, max_len_host, nhead, out, o_stride, mode, stream);
}

// ---- entry points for the fused cross-encoder chains (xenc.hip) --------------------------------
size_t spr::attn_tp(int t, int nseg) { return ::attn_tp_(t, nseg); }
int spr::attn_mode() { return spr::g_attn_mode.load(std::memory_order_relaxed); }
void spr::attn_layout_planes(Workspace& w, int t, int nseg, int d, AttnPlanes& pl) {
  AttnSmall sm{};
  attn_layout(w, t, nseg, d, pl, sm);
}
int spr::attn_zero_gaps(const AttnPlanes& pl, int d, hipStream_t stream) {
  hipLaunchKernelGGL(k_attn_zero_gaps, dim3(d), dim3(256), 0, stream, pl.cu, pl.nseg, pl.tp, pl.vth, pl.vtl);
  SPR_LAUNCH_CHECK();
  return 0;
}
int spr::attn_core_on_planes(const AttnPlanes& pl, const int* kv_seg, int max_len_host, int nhead, float* out,
                             int o_stride, int mode, hipStream_t stream, const int* o_tiles) {
  SPR_REQUIRE(mode >= 1 && mode <= 4, "attention core on planes: mode must be 1 .. 4 (got %d)", mode);
  SPR_REQUIRE((long)cdiv(max_len_host, QB) * nhead * pl.nseg < (1l << 31), "attention: grid too large");
  SPR_REQUIRE(o_tiles == nullptr || nhead == 8, "attention core: tiled output needs 8 heads (got %d)", nhead);
  return launch_core(pl, pl.t_total, (size_t)pl.tp, pl.cu, kv_seg, pl.nseg, max_len_host, nhead, out, o_stride, mode,
                     stream, nullptr, o_tiles);
}

extern "C" int spr_set_attn_mode(int mode) {
  SPR_REQUIRE(mode >= 0 && mode <= 4,
              "attention mode must be 0 (exact f32 MFMA), 1 (split-fp16), 2 (single-pass fp16), 3 (split-fp16 "
              "scores, one probability plane) or 4 (as 1, the lo plane of the probabilities only on significant tiles)");
  spr::g_attn_mode.store(mode);
  return 0;
}
