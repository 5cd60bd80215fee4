// Learned positional embedding (spr_posemb_mlp, spr_posemb_mlp_bwd): the MLP 3 -> 32 -> 64 -> 128 -> 256 -> 256 with a
// ReLU behind each of the first four layers, PositionEmbeddingLearned of models/transformer/position_embedding.py:53-72.
//
// Forward: ONE kernel.  A workgroup of 8 waves owns a tile of 64 tokens and carries it through all five layers; the
// activations live in two LDS buffers (k-major, [channel][token], so that an MFMA A fragment is a conflict-free read)
// that alternate as a layer's input and output.  Nothing but xyz is read and nothing but the embedding is written.
// The weights (108 640 floats, 434 KB) do not fit beside them: every layer streams its weight matrix through a
// double-buffered LDS slab of 16 contraction rows, the next slab's global loads issued into registers before the
// current slab's matrix instructions (the pipeline of bgemm.hip's large-tile kernel).  All workgroups read the same
// 434 KB, which stay resident in L2.
//
// Arithmetic: exact f32 everywhere.  Layer 1 (k = 3) is three multiplies and adds per output on the VALU; layers 2-5
// run on v_mfma_f32_32x32x2_f32, a k-ordered fp32 accumulation per output like a float32 reference's.  No operand is
// scaled or narrowed, so no magnitude of coordinates or weights needs a bound, and spr_set_gemm_mode does not reach
// these kernels.  Wave w owns output channels [32 w, 32 w + 32) of a layer (waves beyond the layer's width idle in the
// two narrow layers) and all tokens of the tile: 2 accumulators of 32 x 32.
//
// Backward: nothing of the forward is kept but xyz.  k_posemb_mlp_chain recomputes h_1 .. h_4 for a tile of 32 tokens
// (the same layer code), keeps the four ReLU masks as bits in the registers of the lanes that will hold the matching
// delta (a layer's output and the delta arriving at it have the same shape, hence the same accumulator layout), runs
// delta_l = (delta_{l+1} W_{l+1}) * relu'(h_l) back down through the same slab pipeline (weights walked row-wise
// instead of column-wise) and writes h_1 .. h_4 and delta_1 .. delta_4 to the caller's workspace.  The five weight
// gradients dW_l = delta_l^T h_{l-1} then go through spr_bgemm (exact f32, one record per 256 tokens) and
// spr_reduce_parts, the bias gradients through spr_colsum: fixed partitions, fixed summation order, no atomics --
// two calls give the same bits.  Tokens are processed in groups of 16 384 so that the workspace stays bounded.
#include "spr_common.h"
#include "split_mma.h"

namespace spr {
namespace {

constexpr int NT = 512;          // threads per workgroup (8 waves)
constexpr int KB = 16;           // contraction rows per weight slab
constexpr int LDW = 257;         // slab row stride in floats (256 outputs + 1)
constexpr int kSlabFloats = 2 * KB * LDW;

struct PmParams {
  const float* w[5];
  const float* b[5];
};

// acc[mi] = A B over K.  A(token, k) = src[k * LDA + token] in LDS (LDA = 32 MI + 1); B(k, n) = W[n * K + k]
// (TRANS = false: y = h W^T of nn.Linear) or W[k * N + n] (TRANS = true: the backward's delta W).  Contains barriers:
// every thread of the workgroup calls it; the first barrier also orders the caller's writes to src before the reads.
template <int MI, int K, int N, bool TRANS>
__device__ __forceinline__ void mfma_layer(const float* __restrict__ W, const float* src, float* Ws, f32x16 (&acc)[MI]) {
  constexpr int LDA = 32 * MI + 1;
  constexpr int NV4 = KB * N / 4;                    // float4 of one slab
  constexpr int NV = (NV4 + NT - 1) / NT;            // per thread
  static_assert(K % KB == 0 && N % 32 == 0 && N <= 256, "layer shape");
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, lh = lane >> 5;
  const int wn = wave * 32;
  const bool active = wn < N;                        // wave-uniform
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[mi][r] = 0.f;

  float4 rw[NV];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int p = 0; p < NV; ++p) {
      const int e = p * NT + tid;
      if (e < NV4) {
        if (TRANS) {
          const int n4 = e % (N / 4), kk = e / (N / 4);
          rw[p] = *reinterpret_cast<const float4*>(W + (size_t)(k0 + kk) * N + 4 * n4);
        } else {
          const int k4 = e % (KB / 4), n = e / (KB / 4);
          rw[p] = *reinterpret_cast<const float4*>(W + (size_t)n * K + k0 + 4 * k4);
        }
      }
    }
  };
  auto stash = [&](int buf) {
    float* d = Ws + buf * (KB * LDW);
#pragma unroll
    for (int p = 0; p < NV; ++p) {
      const int e = p * NT + tid;
      if (e < NV4) {
        if (TRANS) {
          const int n4 = e % (N / 4), kk = e / (N / 4);
          float* q = d + kk * LDW + 4 * n4;
          q[0] = rw[p].x; q[1] = rw[p].y; q[2] = rw[p].z; q[3] = rw[p].w;
        } else {
          const int k4 = e % (KB / 4), n = e / (KB / 4);
          float* q = d + (4 * k4) * LDW + n;
          q[0] = rw[p].x; q[LDW] = rw[p].y; q[2 * LDW] = rw[p].z; q[3 * LDW] = rw[p].w;
        }
      }
    }
  };
  fetch(0);
  stash(0);
  __syncthreads();
  int buf = 0;
  for (int k0 = 0; k0 < K; k0 += KB, buf ^= 1) {
    const bool more = k0 + KB < K;
    if (more) fetch(k0 + KB);                        // in flight under this slab's matrix instructions
    if (active) {
      const float* wb = Ws + buf * (KB * LDW) + wn + l31;
      const float* ab = src + (size_t)k0 * LDA + l31;
#pragma unroll
      for (int s2 = 0; s2 < KB / 2; ++s2) {
        const float b = wb[(2 * s2 + lh) * LDW];
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
          const float a = ab[(2 * s2 + lh) * LDA + 32 * mi];
          acc[mi] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[mi], 0, 0, 0);
        }
      }
    }
    if (more) stash(buf ^ 1);                        // the other buffer: last read one slab ago, behind a barrier
    __syncthreads();
  }
}

__device__ __forceinline__ float relu(float v) { return v < 0.f ? 0.f : v; }   // NaN stays NaN, as in torch

// Layer 1 in the accumulator layout of the MFMA layers, by wave 0: h1[c][token] = relu(w[c] . xyz[token] + b[c]).
// xs = the tile's coordinates in LDS ([token][3], zeros behind the last token).  h (or NULL) = the global copy of the
// layer's output, `valid` tokens from row 0 on; mask receives bit mi * 16 + r = h > 0.
template <int MI>
__device__ __forceinline__ void layer1(const PmParams& p, const float* xs, float* dst, float* __restrict__ h, int valid,
                                       unsigned& mask) {
  constexpr int LDA = 32 * MI + 1;
  mask = 0u;
  if (threadIdx.x >= 64) return;
  const int c = threadIdx.x & 31, lh = threadIdx.x >> 5;
  const float w0 = p.w[0][3 * c], w1 = p.w[0][3 * c + 1], w2 = p.w[0][3 * c + 2], b = p.b[0][c];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int t = acc_row32(r, lh, 32 * mi);
      const float v = relu(((w0 * xs[3 * t] + w1 * xs[3 * t + 1]) + w2 * xs[3 * t + 2]) + b);
      dst[c * LDA + t] = v;
      if (v > 0.f) mask |= 1u << (16 * mi + r);
      if (h != nullptr && t < valid) h[(size_t)t * 32 + c] = v;
    }
}

// acc + bias -> ReLU -> the next layer's LDS input (dst, or NULL) and the global copy (h, or NULL); mask as in layer1.
template <int MI, int N>
__device__ __forceinline__ void epilogue_fwd(const f32x16 (&acc)[MI], const float* __restrict__ bias, float* dst,
                                             float* __restrict__ h, int valid, unsigned& mask) {
  constexpr int LDA = 32 * MI + 1;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l31 = lane & 31, lh = lane >> 5;
  mask = 0u;
  if (wave * 32 >= N) return;
  const int n = wave * 32 + l31;
  const float b = bias[n];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int t = acc_row32(r, lh, 32 * mi);
      const float v = relu(acc[mi][r] + b);
      if (dst != nullptr) dst[n * LDA + t] = v;
      if (v > 0.f) mask |= 1u << (16 * mi + r);
      if (h != nullptr && t < valid) h[(size_t)t * N + n] = v;
    }
}

// delta = relu'(h) * acc (relu'(0) = 0) -> the next product's LDS input (dst, or NULL) and the global copy.
template <int N>
__device__ __forceinline__ void epilogue_bwd(const f32x16 (&acc)[1], unsigned mask, float* dst, float* __restrict__ dl,
                                             int valid) {
  constexpr int LDA = 33;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l31 = lane & 31, lh = lane >> 5;
  if (wave * 32 >= N) return;
  const int n = wave * 32 + l31;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int t = acc_row32(r, lh);
    const float v = (mask >> r) & 1u ? acc[0][r] : 0.f;
    if (dst != nullptr) dst[n * LDA + t] = v;
    if (t < valid) dl[(size_t)t * N + n] = v;
  }
}

// the tile's coordinates -> LDS, zeros behind token T
template <int TT>
__device__ __forceinline__ void stage_xyz(const float* __restrict__ xyz, int t0, int T, float* xs) {
  for (int e = threadIdx.x; e < 3 * TT; e += NT) xs[e] = t0 + e / 3 < T ? xyz[(size_t)3 * t0 + e] : 0.f;
  __syncthreads();
}

constexpr int kFwdTT = 64, kFwdLDA = kFwdTT + 1;
constexpr size_t kFwdLds = ((128 + 256) * kFwdLDA + kSlabFloats + 3 * kFwdTT) * sizeof(float);   // 133 504 bytes

__global__ __launch_bounds__(NT) void k_posemb_mlp_fwd(const float* __restrict__ xyz, PmParams p, int T,
                                                       float* __restrict__ pe) {
  extern __shared__ float sm[];
  float* P = sm;                          // 128 channels: h1, h3
  float* Q = P + 128 * kFwdLDA;           // 256 channels: h2, h4
  float* Ws = Q + 256 * kFwdLDA;
  float* xs = Ws + kSlabFloats;
  const int t0 = blockIdx.x * kFwdTT;
  unsigned mask;
  stage_xyz<kFwdTT>(xyz, t0, T, xs);
  layer1<2>(p, xs, P, nullptr, 0, mask);
  f32x16 acc[2];
  mfma_layer<2, 32, 64, false>(p.w[1], P, Ws, acc);
  epilogue_fwd<2, 64>(acc, p.b[1], Q, nullptr, 0, mask);
  mfma_layer<2, 64, 128, false>(p.w[2], Q, Ws, acc);
  epilogue_fwd<2, 128>(acc, p.b[2], P, nullptr, 0, mask);
  mfma_layer<2, 128, 256, false>(p.w[3], P, Ws, acc);
  epilogue_fwd<2, 256>(acc, p.b[3], Q, nullptr, 0, mask);
  mfma_layer<2, 256, 256, false>(p.w[4], Q, Ws, acc);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, lh = lane >> 5;
  const int n = wave * 32 + (lane & 31);
  const float b = p.b[4][n];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int t = acc_row32(r, lh, t0 + 32 * mi);
      if (t < T) pe[(size_t)t * 256 + n] = acc[mi][r] + b;
    }
}

constexpr int kBwdTT = 32, kBwdLDA = kBwdTT + 1;
constexpr size_t kBwdLds = (2 * 256 * kBwdLDA + kSlabFloats + 3 * kBwdTT) * sizeof(float);       // 100 864 bytes

// h1 [T,32], h2 [T,64], h3 [T,128], h4 [T,256], d1 .. d4 likewise; dpe [T,256] is delta_5.
__global__ __launch_bounds__(NT) void k_posemb_mlp_chain(const float* __restrict__ xyz, PmParams p,
                                                         const float* __restrict__ dpe, int T, float* __restrict__ h1,
                                                         float* __restrict__ h2, float* __restrict__ h3,
                                                         float* __restrict__ h4, float* __restrict__ d1,
                                                         float* __restrict__ d2, float* __restrict__ d3,
                                                         float* __restrict__ d4) {
  extern __shared__ float sm[];
  float* P = sm;
  float* Q = P + 256 * kBwdLDA;
  float* Ws = Q + 256 * kBwdLDA;
  float* xs = Ws + kSlabFloats;
  const int t0 = blockIdx.x * kBwdTT;
  const int valid = T - t0 < kBwdTT ? T - t0 : kBwdTT;
  unsigned m1, m2, m3, m4;
  f32x16 acc[1];
  // ---- the forward chain again
  stage_xyz<kBwdTT>(xyz, t0, T, xs);
  layer1<1>(p, xs, P, h1 + (size_t)t0 * 32, valid, m1);
  mfma_layer<1, 32, 64, false>(p.w[1], P, Ws, acc);
  epilogue_fwd<1, 64>(acc, p.b[1], Q, h2 + (size_t)t0 * 64, valid, m2);
  mfma_layer<1, 64, 128, false>(p.w[2], Q, Ws, acc);
  epilogue_fwd<1, 128>(acc, p.b[2], P, h3 + (size_t)t0 * 128, valid, m3);
  mfma_layer<1, 128, 256, false>(p.w[3], P, Ws, acc);
  epilogue_fwd<1, 256>(acc, p.b[3], nullptr, h4 + (size_t)t0 * 256, valid, m4);
  // ---- delta_5 = dpe -> P (every read of P ended behind the last barrier of the layer above)
  for (int e = threadIdx.x; e < kBwdTT * 64; e += NT) {
    const int t = e >> 6, j4 = e & 63;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (t < valid) v = *reinterpret_cast<const float4*>(dpe + (size_t)(t0 + t) * 256 + 4 * j4);
    float* q = P + (4 * j4) * kBwdLDA + t;
    q[0] = v.x; q[kBwdLDA] = v.y; q[2 * kBwdLDA] = v.z; q[3 * kBwdLDA] = v.w;
  }
  // ---- back down
  mfma_layer<1, 256, 256, true>(p.w[4], P, Ws, acc);
  epilogue_bwd<256>(acc, m4, Q, d4 + (size_t)t0 * 256, valid);
  mfma_layer<1, 256, 128, true>(p.w[3], Q, Ws, acc);
  epilogue_bwd<128>(acc, m3, P, d3 + (size_t)t0 * 128, valid);
  mfma_layer<1, 128, 64, true>(p.w[2], P, Ws, acc);
  epilogue_bwd<64>(acc, m2, Q, d2 + (size_t)t0 * 64, valid);
  mfma_layer<1, 64, 32, true>(p.w[1], Q, Ws, acc);
  epilogue_bwd<32>(acc, m1, nullptr, d1 + (size_t)t0 * 32, valid);
}

// ---- weight-gradient products: one spr_bgemm record per kSlab tokens ------------------------------
constexpr int kGroup = 16384;    // tokens whose activations and deltas the workspace holds at a time
constexpr int kSlab = 256;       // tokens per split-K record
constexpr int kMaxSlab = kGroup / kSlab;
// layer widths: 3, 32, 64, 128, 256, 256
__host__ __device__ constexpr int width(int l) { return l == 0 ? 3 : (l >= 4 ? 256 : 16 << l); }

struct PmDesc {                  // the record layout of spr_bgemm (include/spr.h)
  long long a_off, b_off, c_off;
  int m, n, k, pad;
};

// desc[l][s]: dW_l part s = delta_l[s kSlab ..]^T h_{l-1}[s kSlab ..] of a group of `rows` tokens
__global__ void k_posemb_mlp_desc(PmDesc* __restrict__ desc, int rows) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 5 * kMaxSlab) return;
  const int l = i / kMaxSlab, s = i % kMaxSlab;
  const int k_in = width(l), n_out = width(l + 1);
  const int left = rows - s * kSlab;
  PmDesc d;
  d.a_off = (long long)s * kSlab * n_out;
  d.b_off = (long long)s * kSlab * k_in;
  d.c_off = (long long)s * n_out * k_in;
  d.m = n_out;
  d.n = k_in;
  d.k = left < 0 ? 0 : (left < kSlab ? left : kSlab);
  d.pad = 0;
  desc[i] = d;
}

struct BwdWorkspace {
  float *h[5], *d[5], *parts[5], *btmp;
  PmDesc* desc;
  void* colws;
  size_t colws_bytes;
};

int group_rows(int t) { return t < kGroup ? (t + 31) / 32 * 32 : kGroup; }

BwdWorkspace bwd_layout(Workspace& a, int t) {
  BwdWorkspace w;
  const size_t g = (size_t)group_rows(t);
  const int nslab = (int)((g + kSlab - 1) / kSlab);
  for (int l = 1; l <= 4; ++l) {
    w.h[l] = a.take<float>(g * width(l));
    w.d[l] = a.take<float>(g * width(l));
  }
  for (int l = 0; l < 5; ++l) w.parts[l] = a.take<float>((size_t)nslab * width(l) * width(l + 1));
  w.btmp = a.take<float>(256);
  w.desc = a.take<PmDesc>(5 * kMaxSlab);
  w.colws_bytes = spr_colsum_workspace_bytes(256);
  w.colws = a.take<char>(w.colws_bytes);
  return w;
}

int check_common(const char* what, const float* xyz, const float* const* params_host, int t, int d_model) {
  SPR_REQUIRE(t >= 0, "%s: negative token count %d", what, t);
  SPR_REQUIRE(d_model == 256, "%s: d_model must be 256 (got %d): the widths 3/32/64/128/256/d_model are fixed", what,
              d_model);
  SPR_REQUIRE(params_host != nullptr, "%s: null parameter list", what);
  for (int i = 0; i < 10; ++i)
    SPR_REQUIRE(params_host[i] != nullptr && ((uintptr_t)params_host[i] & 15) == 0,
                "%s: parameter %d is null or not 16-byte aligned", what, i);
  SPR_REQUIRE(t == 0 || xyz != nullptr, "%s: null xyz", what);
  return 0;
}

PmParams pack(const float* const* params_host) {
  PmParams p;
  for (int l = 0; l < 5; ++l) {
    p.w[l] = params_host[2 * l];
    p.b[l] = params_host[2 * l + 1];
  }
  return p;
}

}  // namespace
}  // namespace spr

using namespace spr;

extern "C" int spr_posemb_mlp(const float* xyz, const float* const* params_host, int t, int d_model, float* pe,
                              void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (int rc = check_common("posemb_mlp", xyz, params_host, t, d_model)) return rc;
  if (t == 0) return 0;
  SPR_REQUIRE(pe != nullptr, "posemb_mlp: null output");
  SPR_REQUIRE(t <= (1 << 30), "posemb_mlp: too many tokens (%d)", t);
  if (int rc = ensure_dyn_lds((const void*)k_posemb_mlp_fwd, (int)kFwdLds)) return rc;
  hipLaunchKernelGGL(k_posemb_mlp_fwd, dim3(cdiv(t, kFwdTT)), dim3(NT), kFwdLds, stream, xyz, pack(params_host), t, pe);
  SPR_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t spr_posemb_mlp_bwd_workspace_bytes(int t) {
  if (t <= 0) return 256;
  return measure(bwd_layout, t);
}

extern "C" int spr_posemb_mlp_bwd(const float* xyz, const float* const* params_host, const float* dpe, int t,
                                  int d_model, float* const* grads_host, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (int rc = check_common("posemb_mlp_bwd", xyz, params_host, t, d_model)) return rc;
  SPR_REQUIRE(grads_host != nullptr, "posemb_mlp_bwd: null gradient list");
  for (int i = 0; i < 10; ++i) SPR_REQUIRE(grads_host[i] != nullptr, "posemb_mlp_bwd: gradient %d is null", i);
  if (t == 0) {   // an empty sum
    for (int l = 0; l < 5; ++l) {
      SPR_HIP_CHECK(hipMemsetAsync(grads_host[2 * l], 0, sizeof(float) * width(l) * width(l + 1), stream));
      SPR_HIP_CHECK(hipMemsetAsync(grads_host[2 * l + 1], 0, sizeof(float) * width(l + 1), stream));
    }
    return 0;
  }
  SPR_REQUIRE(dpe != nullptr && ((uintptr_t)dpe & 15) == 0, "posemb_mlp_bwd: dpe is null or not 16-byte aligned");
  SPR_REQUIRE(t <= (1 << 30), "posemb_mlp_bwd: too many tokens (%d)", t);
  Workspace a(ws, ws_bytes);
  const BwdWorkspace w = bwd_layout(a, t);
  SPR_REQUIRE(ws != nullptr && ((uintptr_t)ws & 255) == 0 && a.ok(),
              "posemb_mlp_bwd: workspace too small or misaligned (%zu bytes, need %zu)", ws_bytes,
              spr_posemb_mlp_bwd_workspace_bytes(t));
  if (int rc = ensure_dyn_lds((const void*)k_posemb_mlp_chain, (int)kBwdLds)) return rc;
  const PmParams p = pack(params_host);
  for (int g0 = 0, g = 0; g0 < t; g0 += kGroup, ++g) {
    const int rows = t - g0 < kGroup ? t - g0 : kGroup;
    const int nslab = cdiv(rows, kSlab);
    const float* dpe_g = dpe + (size_t)g0 * 256;
    hipLaunchKernelGGL(k_posemb_mlp_chain, dim3(cdiv(rows, kBwdTT)), dim3(NT), kBwdLds, stream, xyz + (size_t)g0 * 3, p,
                       dpe_g, rows, w.h[1], w.h[2], w.h[3], w.h[4], w.d[1], w.d[2], w.d[3], w.d[4]);
    SPR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_posemb_mlp_desc, dim3(cdiv(5 * kMaxSlab, 64)), dim3(64), 0, stream, w.desc, rows);
    SPR_LAUNCH_CHECK();
    for (int l = 0; l < 5; ++l) {
      const int k_in = width(l), n_out = width(l + 1);
      const float* delta = l == 4 ? dpe_g : w.d[l + 1];
      const float* hin = l == 0 ? xyz + (size_t)g0 * 3 : w.h[l];
      // dW_l[n, k] = sum_t delta[t, n] hin[t, k]: A(i = n, k = t) = delta, B(k = t, j = k) = hin
      if (int rc = spr_bgemm(delta, hin, w.parts[l], w.desc + l * kMaxSlab, nslab, n_out, k_in, 1, n_out, k_in, 1, k_in,
                             1, 1.0f, 0.0f, stream_))
        return rc;
      if (int rc = spr_reduce_parts(w.parts[l], nslab, (long)n_out * k_in, 1.0f, grads_host[2 * l], g > 0, stream_))
        return rc;
      if (int rc = spr_colsum(delta, rows, n_out, w.btmp, w.colws, w.colws_bytes, stream_)) return rc;
      if (int rc = spr_reduce_parts(w.btmp, 1, n_out, 1.0f, grads_host[2 * l + 1], g > 0, stream_)) return rc;
    }
  }
  return 0;
}
