// Decoder projection with the nearest-upsample gather and the skip concatenation folded into the GEMM's staging.
//
// Behaviour contract:
//   NearestUpsampleBlock.forward -> closest_pool (kpconv_blocks.py:757-768, :112-124), the torch.cat of
//   KPFDecoder.forward (kpconv.py:156-158) and UnaryBlock.mlp (kpconv_blocks.py:549,:557):
//     y[i, :] = [ xc[idx0[i], :] | xs[i, :] ] . W^T        idx0[i] = idx[i * idx_stride]
//   A row whose index lies outside [0, nc) contributes a zero coarse row (closest_pool's appended zero row).
//
// The NT GEMM of linear.hip with two row sources for the X operand: K slabs 0 .. kc / 32 - 1 come from the gathered
// rows of xc, the remaining ks / 32 from the rows of xs.  Every thread keeps the row numbers of the float4s it stages
// in registers for the whole tile (the coarse one clamped into xc, with a flag for "zero row"), so the gather costs
// one index read per staged row and tile and nothing per slab.  A zero row is loaded from the clamped address and
// replaced by zeros behind the wait, in front of the split: no lane ever forms an address outside xc and the
// inline-asm loads stay unconditional.
//   k_upun_h3  (spr_set_gemm_mode 1)  split-fp16 operands, three MFMAs per k-step (split_mma.h); xc and xs share ONE
//     power-of-two scale, taken from the larger of their two ranges: the result is the one spr_linear gives on the
//     concatenated tensor.  One partial of max |y| per workgroup is published like spr_linear's.
//   k_upun_f32 (mode 0)               exact-f32 matrix cores, a k-ordered fmaf chain over the kc + ks columns.
// Fixed reduction order (k ascending), no atomics: a row's bits depend on its own operands and the scales only.
#include "attn_planes.h"
#include "lds_dma.h"
#include "spr_common.h"
#include "split_mma.h"

namespace spr {
namespace {

constexpr int BK = kPlaneK;
constexpr int LDSK = BK + 1;

// The staged rows of one thread: float4 number f = tid + i NT of a [ROWS][32 k] slab is row f / 8, columns 4 (f % 8).
template <int ROWS, int NT>
struct RowMap {
  static constexpr int PT = ROWS * (BK / 4) / NT;
  static_assert(ROWS * (BK / 4) % NT == 0, "slab must divide over the threads");
  int fine[PT];     // row of xs, clamped to n - 1
  int coarse[PT];   // row of xc, clamped into [0, nc)
  bool live[PT];    // the coarse row exists
  __device__ __forceinline__ void init(const int* __restrict__ idx, int idx_stride, int m0, int n, int nc, int tid) {
#pragma unroll
    for (int i = 0; i < PT; ++i) {
      const int r = (tid + i * NT) / (BK / 4);
      fine[i] = min(m0 + r, n - 1);
      const int g = idx[(size_t)fine[i] * idx_stride];
      live[i] = g >= 0 && g < nc;
      coarse[i] = live[i] ? g : 0;
    }
  }
};

// the gathered twin of slab_load (split_mma.h): rows from the map, columns k0 .. k0 + 31 of a row of `ld` floats
template <int PT, int NT>
__device__ __forceinline__ void slab_load_rows(f32x4 (&regs)[PT], const float* __restrict__ X, const int (&rows)[PT],
                                               int ld, int tid, int k0) {
#pragma unroll
  for (int i = 0; i < PT; ++i) {
    const int c4 = (tid + i * NT) % (BK / 4);
    const float* p = X + (size_t)rows[i] * ld + k0 + c4 * 4;
    asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(regs[i]) : "v"(p));
  }
}

template <int BM, int BN, int WM, int WN>
__global__ __launch_bounds__(WM* WN * 64) void k_upun_h3(
    const float* __restrict__ xc, int nc, int kc, const float* __restrict__ xs, int n, int ks,
    const int* __restrict__ idx, int idx_stride, const float* __restrict__ Wt, int N, float* __restrict__ out,
    const float* __restrict__ c_parts, int n_cparts, const float* __restrict__ s_parts, int n_sparts,
    const float* __restrict__ w_parts, int n_wparts, float* __restrict__ out_parts) {
  constexpr int NT = WM * WN * 64;
  constexpr int TM = BM / (WM * 32), TN = BN / (WN * 32);   // 32x32 sub-tiles per wave
  extern __shared__ __align__(16) unsigned char upun_smem[];
  _Float16* Ah = reinterpret_cast<_Float16*>(upun_smem);
  _Float16* Al = Ah + BM * kPlaneStride;
  _Float16* Bh = Al + BM * kPlaneStride;
  _Float16* Bl = Bh + BN * kPlaneStride;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int wm = wave / WN, wn = wave % WN;
  const int K = kc + ks;
  const int gx = (N + BN - 1) / BN;
  const int lid = xcd_swizzle(blockIdx.x, gridDim.x);   // the column tiles of one row panel share an L2
  const int m0 = (lid / gx) * BM, n0 = (lid % gx) * BN;
  const int l31 = lane & 31, lh = lane >> 5;

  float sa, sb, unscale;
  {
    float* shf = reinterpret_cast<float*>(upun_smem);
    const float ac = block_absmax(c_parts, shf, n_cparts);
    const float as = block_absmax(s_parts, shf, n_sparts);
    const int ka = pow2_exp_for(fmaxf(ac, as));           // one scale for both halves of the concatenated row
    const int kb = pow2_exp_for(block_absmax(w_parts, shf, n_wparts));
    __syncthreads();   // shf aliases the operand tiles
    sa = pow2f(ka);
    sb = pow2f(kb);
    unscale = pow2f(-ka - kb);
  }

  RowMap<BM, NT> rows;
  rows.init(idx, idx_stride, m0, n, nc, tid);

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  f32x4 ra[BM * BK / 4 / NT], rb[BN * BK / 4 / NT];
  auto load_slab = [&](int k0) {
    if (k0 < kc) slab_load_rows<RowMap<BM, NT>::PT, NT>(ra, xc, rows.coarse, kc, tid, k0);
    else slab_load_rows<RowMap<BM, NT>::PT, NT>(ra, xs, rows.fine, ks, tid, k0 - kc);
    slab_load<BN, NT>(rb, Wt, N, K, tid, n0, k0);
  };
  auto store_slab = [&](int k0) {
    wait_vm<0>();
    __builtin_amdgcn_sched_barrier(0);
    if (k0 < kc) {
#pragma unroll
      for (int i = 0; i < RowMap<BM, NT>::PT; ++i)
        if (!rows.live[i]) ra[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    slab_store<BM, NT>(ra, sa, Ah, Al, tid);
    slab_store<BN, NT>(rb, sb, Bh, Bl, tid);
  };

  load_slab(0);
  for (int k0 = 0; k0 < K; k0 += BK) {
    store_slab(k0);
    __syncthreads();
    if (k0 + BK < K) load_slab(k0 + BK);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int s = 0; s < BK / 16; ++s) {
      const int ko = 16 * s + 8 * lh;
      f16x8 ah[TM], al[TM], bh[TN], bl[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) frag_ld40(Ah, Al, (wm * TM + i) * 32 + l31, ko, ah[i], al[i]);
#pragma unroll
      for (int j = 0; j < TN; ++j) frag_ld40(Bh, Bl, (wn * TN + j) * 32 + l31, ko, bh[j], bl[j]);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = mma3_32(ah[i], al[i], bh[j], bl[j], acc[i][j]);
    }
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();
  }
  wait_vm<0>();

  float omax = 0.f;
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int col = n0 + (wn * TN + j) * 32 + l31;
    if (col >= N) continue;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int row0 = m0 + (wm * TM + i) * 32;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = row0 + acc_row32(r, lh);
        const float v = acc[i][j][r] * unscale;   // exact power of two
        if (row < n) {
          out[(size_t)row * N + col] = v;
          omax = fmaxf(omax, fabsf(v));
        }
      }
    }
  }
  if (out_parts != nullptr) {
    // max |y| of this tile: the norm behind the projection hands it on without a pass over y
    float* shf = reinterpret_cast<float*>(upun_smem);
    omax = wave_max(omax);
    __syncthreads();
    if (lane == 0) shf[wave] = omax;
    __syncthreads();
    if (tid == 0) {
      float t = shf[0];
      for (int w_ = 1; w_ < WM * WN; ++w_) t = fmaxf(t, shf[w_]);
      out_parts[blockIdx.x] = t;
    }
  }
}

// WM x WN waves, each one 32x32 accumulator of v_mfma_f32_32x32x2_f32; LDS row stride of 33 words.
template <int WM, int WN>
__global__ __launch_bounds__(WM* WN * 64) void k_upun_f32(
    const float* __restrict__ xc, int nc, int kc, const float* __restrict__ xs, int n, int ks,
    const int* __restrict__ idx, int idx_stride, const float* __restrict__ Wt, int N, float* __restrict__ out) {
  constexpr int BM = WM * 32, BN = WN * 32, NT = WM * WN * 64;
  constexpr int B_F4 = BN * BK / 4, B_PT = (B_F4 + NT - 1) / NT;
  __shared__ float As[BM * LDSK];
  __shared__ float Bs[BN * LDSK];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int wm = wave / WN, wn = wave % WN;
  const int K = kc + ks;
  const int gx = (N + BN - 1) / BN;
  const int lid = xcd_swizzle(blockIdx.x, gridDim.x);
  const int m0 = (lid / gx) * BM, n0 = (lid % gx) * BN;
  const int l31 = lane & 31, lh = lane >> 5;

  RowMap<BM, NT> rows;
  constexpr int A_PT = RowMap<BM, NT>::PT;
  rows.init(idx, idx_stride, m0, n, nc, tid);

  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;

  f32x4 ra[A_PT], rb[B_PT];
  auto load_slab = [&](int k0) {
    if (k0 < kc) slab_load_rows<A_PT, NT>(ra, xc, rows.coarse, kc, tid, k0);
    else slab_load_rows<A_PT, NT>(ra, xs, rows.fine, ks, tid, k0 - kc);
#pragma unroll
    for (int i = 0; i < B_PT; ++i) {
      const int f = tid + i * NT;
      if (f < B_F4) {
        const int r = f / (BK / 4), c4 = f % (BK / 4);
        const float* p = Wt + (size_t)min(n0 + r, N - 1) * K + k0 + c4 * 4;
        asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(rb[i]) : "v"(p));
      }
    }
  };
  auto store_slab = [&](int k0) {
    wait_vm<0>();
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < A_PT; ++i) {
      const int f = tid + i * NT;
      const int r = f / (BK / 4), c4 = f % (BK / 4);
      const bool in = m0 + r < n && (k0 >= kc || rows.live[i]);   // rows past n and zero rows contribute zeros
      float* d = As + r * LDSK + c4 * 4;
      d[0] = in ? ra[i][0] : 0.f;
      d[1] = in ? ra[i][1] : 0.f;
      d[2] = in ? ra[i][2] : 0.f;
      d[3] = in ? ra[i][3] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < B_PT; ++i) {
      const int f = tid + i * NT;
      if (f < B_F4) {
        const int r = f / (BK / 4), c4 = f % (BK / 4);
        const bool in = n0 + r < N;
        float* d = Bs + r * LDSK + c4 * 4;
        d[0] = in ? rb[i][0] : 0.f;
        d[1] = in ? rb[i][1] : 0.f;
        d[2] = in ? rb[i][2] : 0.f;
        d[3] = in ? rb[i][3] : 0.f;
      }
    }
  };

  load_slab(0);
  for (int k0 = 0; k0 < K; k0 += BK) {
    store_slab(k0);
    __syncthreads();
    if (k0 + BK < K) load_slab(k0 + BK);
    __builtin_amdgcn_sched_barrier(0);
    const float* ap = As + (wm * 32 + l31) * LDSK + lh;
    const float* bp = Bs + (wn * 32 + l31) * LDSK + lh;
    float fa[BK / 2], fb[BK / 2];
#pragma unroll
    for (int s = 0; s < BK / 2; ++s) {
      fa[s] = ap[2 * s];
      fb[s] = bp[2 * s];
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int s = 0; s < BK / 2; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[s], fb[s], acc, 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();
  }
  wait_vm<0>();
  const int col = n0 + wn * 32 + l31;
  if (col >= N) return;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = m0 + wm * 32 + acc_row32(r, lh);
    if (row < n) out[(size_t)row * N + col] = acc[r];
  }
}

struct UpunWs {
  float *cp, *sp, *wp;   // max |xc|, max |xs|, max |w| partials
};
UpunWs upun_layout(Workspace& w) {
  UpunWs l;
  l.cp = w.take<float>(kAmaxParts);
  l.sp = w.take<float>(kAmaxParts);
  l.wp = w.take<float>(kAmaxParts);
  return l;
}

bool upun_shape_ok(int kc, int ks, int n_out) {
  return kc >= BK && ks >= BK && kc % BK == 0 && ks % BK == 0 && n_out >= 32 && kc <= (1 << 20) && ks <= (1 << 20);
}

}  // namespace
}  // namespace spr

using namespace spr;

extern "C" int spr_upsample_unary_supported(int kc, int ks, int n_out) {
  // Shapes the fused call is the host layer's DEFAULT for: those with a kernel.  Measured against gather + two
  // projections at kc = 256 / 512 / 1024, ks = kc / 2, n_out = ks and kc (profiles/decoder_bench.txt): faster at all
  // six, by 0.9 - 2.6 ms against a spread of at most 0.04 ms, so no shape with a kernel is sent the other way.
  return upun_shape_ok(kc, ks, n_out) ? 1 : 0;
}

extern "C" size_t spr_upsample_unary_workspace_size(void) { return measure(upun_layout); }

extern "C" int spr_upsample_unary(const float* xc, int nc, int kc, const float* xs, int n, int ks, const int* idx,
                                  int idx_stride, const float* w, int n_out, float* y, const float* xc_range,
                                  int xc_range_n, const float* xs_range, int xs_range_n, const float* w_range,
                                  int w_range_n, float* out_range, int out_range_cap, int* out_range_n_host, void* ws,
                                  size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (out_range_n_host) *out_range_n_host = 0;
  SPR_REQUIRE(n >= 0 && nc >= 1 && idx_stride >= 1, "upsample_unary: bad sizes n=%d nc=%d idx_stride=%d", n, nc,
              idx_stride);
  SPR_REQUIRE(upun_shape_ok(kc, ks, n_out),
              "upsample_unary: no kernel for kc=%d ks=%d n_out=%d (kc, ks multiples of 32, n_out >= 32)", kc, ks, n_out);
  SPR_REQUIRE(xc_range == nullptr || xc_range_n >= 1, "upsample_unary: xc_range needs a count");
  SPR_REQUIRE(xs_range == nullptr || xs_range_n >= 1, "upsample_unary: xs_range needs a count");
  SPR_REQUIRE(w_range == nullptr || w_range_n >= 1, "upsample_unary: w_range needs a count");
  if (spr::gemm_mode() == 1) {
    Workspace wk(ws, ws_bytes);
    const auto [cp, sp, wp] = upun_layout(wk);
    SPR_REQUIRE(ws != nullptr && wk.ok(),
                "upsample_unary: workspace too small (%zu bytes given, spr_upsample_unary_workspace_size() needed)",
                ws_bytes);
    if (n == 0) return 0;
    const float* c_parts = xc_range != nullptr ? xc_range : cp;
    const float* s_parts = xs_range != nullptr ? xs_range : sp;
    const float* w_parts = w_range != nullptr ? w_range : wp;
    const int n_cp = xc_range != nullptr ? xc_range_n : kAmaxParts;
    const int n_sp = xs_range != nullptr ? xs_range_n : kAmaxParts;
    const int n_wp = w_range != nullptr ? w_range_n : kAmaxParts;
    // a range measured here covers all of xc, gathered or not: an upper bound of what the tiles stage
    if (xc_range == nullptr && xs_range == nullptr) {
      if (int rc = launch_absmax2(xc, nc, kc, kc, cp, xs, n, ks, ks, sp, stream)) return rc;
    } else if (xc_range == nullptr) {
      if (int rc = launch_absmax(xc, nc, kc, kc, cp, stream)) return rc;
    } else if (xs_range == nullptr) {
      if (int rc = launch_absmax(xs, n, ks, ks, sp, stream)) return rc;
    }
    if (w_range == nullptr) {
      if (int rc = launch_absmax(w, n_out, kc + ks, kc + ks, wp, stream)) return rc;
    }
    auto lds = [](int bm, int bn) { return (size_t)(bm + bn) * spr::kPlaneStride * 2 * sizeof(_Float16); };
    if (n_out % 128 == 0) {
      // 128x128 tiles: at the decoder's widths one workgroup covers the whole output row (n_out = 128) or half of it,
      // so a gathered row is staged once or twice, not once per 64 columns
      const int grid = cdiv(n_out, 128) * cdiv(n, 128);
      float* op = (out_range && grid <= out_range_cap) ? out_range : nullptr;
      if (op && out_range_n_host) *out_range_n_host = grid;
      hipLaunchKernelGGL((spr::k_upun_h3<128, 128, 4, 1>), dim3(grid), dim3(256), lds(128, 128), stream, xc, nc, kc, xs,
                         n, ks, idx, idx_stride, w, n_out, y, c_parts, n_cp, s_parts, n_sp, w_parts, n_wp, op);
    } else {
      const int grid = cdiv(n_out, 64) * cdiv(n, 128);
      float* op = (out_range && grid <= out_range_cap) ? out_range : nullptr;
      if (op && out_range_n_host) *out_range_n_host = grid;
      hipLaunchKernelGGL((spr::k_upun_h3<128, 64, 4, 1>), dim3(grid), dim3(256), lds(128, 64), stream, xc, nc, kc, xs,
                         n, ks, idx, idx_stride, w, n_out, y, c_parts, n_cp, s_parts, n_sp, w_parts, n_wp, op);
    }
  } else {
    if (n == 0) return 0;
    if (n_out % 64 == 0)
      hipLaunchKernelGGL((spr::k_upun_f32<2, 2>), dim3((n_out / 64) * cdiv(n, 64)), dim3(256), 0, stream, xc, nc, kc,
                         xs, n, ks, idx, idx_stride, w, n_out, y);
    else
      hipLaunchKernelGGL((spr::k_upun_f32<4, 1>), dim3(cdiv(n_out, 32) * cdiv(n, 128)), dim3(256), 0, stream, xc, nc,
                         kc, xs, n, ks, idx, idx_stride, w, n_out, y);
  }
  SPR_LAUNCH_CHECK();
  return 0;
}
