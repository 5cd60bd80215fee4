// Deformable / modulated KPConv (linear influence, sum aggregation) on gfx950: forward and the three non-GEMM pieces of
// the backward.  The kernel points move per query by an offset the caller computed (a rigid KPConv + bias).
//
// Behaviour contract: KPConv.forward with deformable=True, models/backbone_kpconv/kpconv_blocks.py:309-412, with K kernel
// points kp, extent e, offset features of [nq, 3K (+ K when modulated)] and y = s[idx[n,k]] - q[n]:
//     :316-322  D[n,p,:] = kp[p] + e of[n, 3p:3p+3];   m[n,p] = 2 sigmoid(of[n, 3K+p]) when modulated, else 1
//     :325-329  d2[n,k,p] = |y - D[n,p]|^2                                          (float32)
//     :337-356  in_range[n,k] = any_p d2 < e^2; only those neighbours are kept (a shadow entry, index outside [0, ns),
//               never is)
//     :369      h = max(0, 1 - sqrt(d2) / e)
//     :388-406  wf[n,p,:] = m[n,p] sum_k h[n,k,p] x[idx[n,k],:];  out[n,:] = sum_p wf[n,p,:] W[p]
//     :409-412  out /= max(1, #{k : in_range[n,k] and sum_c x[idx[n,k],c] > 0})     (the rigid rule counts every valid k)
//     :332      min_d2[n,p] = min_k d2[n,k,p]; a shadow entry takes part as the point (1e6, 1e6, 1e6)
// The count comes from launch_rowflag (kpconv.hip): one summation order of the sign test in the whole library.
//
// Backward pieces, with dWFm = (dout / count) W_flat^T [nq, K cin] from the caller:
//     dx[idx[n,k], c] += sum_p h[n,k,p] m[n,p] dWFm[n,p,c]                          (64-bit fixed point: fx_scatter.h)
//     g[n,k,p]  = sum_c dWFm[n,p,c] x[idx[n,k],c]
//     d of[n, 3p:3p+3] = e m[n,p] sum_k g[n,k,p] (y - D[n,p]) / (sqrt(d2) e)         over items with 0 < sqrt(d2) < e
//     d of[n, 3K+p]    = (sum_k h[n,k,p] g[n,k,p]) 2 s (1 - s),  s = sigmoid(of[n, 3K+p])
// An item with d2 == 0 contributes 0 to d of (the reference's sqrt has no finite derivative there: it yields NaN).
// No gradient reaches the points or the count.
//
// Forward: k_kpconv_deform_tile<CC>, k_kpconv_modes_tile's structure (one workgroup of 8 waves per tile of 32 queries,
//   phase 1 lane = neighbour then lane = channel, phase 2 the split-fp16 MFMA triple against the planes of
//   spr_kpconv_prep_weights).  What differs: a query's 15 deformed kernel points and modulations are formed once per
//   (query, channel chunk) by 15 lanes and parked in LDS (one float4 each; every lane then reads them as broadcasts);
//   only in-range neighbours are staged, so the channel walk skips the about half of a deformable level's row that is out
//   of range; the sums are multiplied by m before they are split (operand bound 2 kmax max|x|: m < 2, h <= 1).
//   LDS at CC = 64: the modes kernel's 156 KB + 8 x 16 float4 = 2 KB; nothing in it grows with kmax.
// Other shapes (cin or cout no multiple of 32, cout > 256, n_kp != 15) and impl == 1: k_kpconv_deform_simple, one thread
//   per output element.  min_d2: k_kpconv_deform_min_d2, one thread per (query, kernel point), only when asked for.
// Backward: k_kpconv_deform_aux<DX> (one wave per query: wf + count, or the scatter) and k_kpconv_deform_offsets (one
//   wave per query, lane = neighbour with one g accumulator per kernel point, dWFm broadcast from LDS 64 channels at a
//   time; the 4 K sums over neighbours are per-lane partials in row order, then wave reductions: no atomics).
#include "spr_common.h"
#include "fx_scatter.h"
#include "split_mma.h"
#include "kpconv_walk.h"

namespace spr {
namespace {

constexpr int kKP = 15;             // kernel points of the tile kernel
constexpr int kKPmax = kWalkKP;     // kernel points at most
constexpr float kFarPoint = 1e6f;   // the reference's shadow point (min_d2 only)

struct DeformArgs {
  const float* kpts;
  int n_kp;
  float extent, inv_extent, e2;
  const float* of;   // [nq, of_stride]: 3 n_kp offsets, then n_kp modulation logits when modulated
  int of_stride, modulated;
};

// Lanes 0 .. n_kp-1 form the query's deformed kernel points and modulations: dq[p] = (D, m).  Fenced on both sides (a
// wave's LDS operations retire in order; the fences keep the compiler from moving them).
__device__ __forceinline__ void form_query(const DeformArgs& a, size_t n, int lane, float4* __restrict__ dq) {
  __builtin_amdgcn_wave_barrier();
  if (lane < a.n_kp) {
    const float* o = a.of + n * a.of_stride;
    float4 v;
    v.x = a.kpts[3 * lane] + a.extent * o[3 * lane];
    v.y = a.kpts[3 * lane + 1] + a.extent * o[3 * lane + 1];
    v.z = a.kpts[3 * lane + 2] + a.extent * o[3 * lane + 2];
    v.w = a.modulated ? 2.f / (1.f + expf(-o[3 * a.n_kp + lane])) : 1.f;
    dq[lane] = v;
  }
  __builtin_amdgcn_wave_barrier();
}

// Lane = one neighbour: its influences against the query's kernel points -> LDS, IN-RANGE neighbours compacted in row
// order; cnt += in-range neighbours whose flag is set; returns the number staged (wave uniform).
__device__ __forceinline__ int stage_deform(const KpNeighbour& nb, const DeformArgs& a, const float4* __restrict__ dq,
                                            float* __restrict__ infl, int* __restrict__ ids, int lane, int& cnt) {
  float w[kKPmax];
  bool keep = false;
#pragma unroll
  for (int p = 0; p < kKPmax; ++p) w[p] = 0.f;
  if (nb.id >= 0) {
#pragma unroll
    for (int p = 0; p < kKPmax; ++p) {
      if (p < a.n_kp) {
        const float4 d = dq[p];
        const float dx = nb.px - d.x, dy = nb.py - d.y, dz = nb.pz - d.z;
        const float d2 = dx * dx + dy * dy + dz * dz;
        w[p] = influence_of<SPR_KP_LINEAR>(d2, a.inv_extent, 0.f);
        keep |= d2 < a.e2;
      }
    }
  }
  const unsigned long long m = __ballot(keep);
  cnt += __popcll(__ballot(keep && nb.pos != 0));
  const int slot = __popcll(m & ((1ull << lane) - 1ull));
  __builtin_amdgcn_wave_barrier();
  if (keep) {
    ids[slot] = nb.id;
#pragma unroll
    for (int p4 = 0; p4 < kKPmax / 4; ++p4)
      *reinterpret_cast<float4*>(infl + slot * kSlot + 4 * p4) =
          make_float4(w[4 * p4], w[4 * p4 + 1], w[4 * p4 + 2], w[4 * p4 + 3]);
  }
  __builtin_amdgcn_wave_barrier();
  return __popcll(m);
}

// ---------------------------------------------------------------------------
// Fused tile kernel (see the head of the file).
constexpr int kTQ = 32, kWaves = 8;
static inline size_t deform_lds_bytes(int cc) {
  return 2 * sizeof(_Float16) * (size_t)kTQ * (kKP * cc + 16) + sizeof(float4) * kWaves * kKPmax +
         sizeof(float) * kWaves * 64 * kSlot + sizeof(int) * kWaves * 64 + sizeof(int) * kTQ;
}

template <int CC>
__global__ __launch_bounds__(64 * kWaves) void k_kpconv_deform_tile(
    const float* __restrict__ q_xyz, int nq, const float* __restrict__ s_xyz, int ns, const int* __restrict__ nbr,
    int nbr_stride, int kmax, const float* __restrict__ x, int cin, const _Float16* __restrict__ Wh,
    const _Float16* __restrict__ Wl, int cout, DeformArgs a, const unsigned char* __restrict__ flag,
    const float* __restrict__ x_parts, const float* __restrict__ w_parts, int n_xparts, int n_wparts,
    float* __restrict__ out) {
  constexpr int TQ = kTQ, NWV = kWaves, QPW = TQ / NWV;
  constexpr int KW = kKP * CC;       // phase-2 K per chunk
  constexpr int SH = KW + 16;        // LDS row stride in halves (k_kpconv_mfma's: conflict-free fragment reads)
  constexpr int KS = KW / 32;        // 32-deep k-steps per chunk
  constexpr bool HALF = CC == 32;
  constexpr int NTW = 4;             // n-tiles per wave at most (cout <= 256)
  static_assert(CC == 32 || CC == 64, "channel chunk");
  extern __shared__ __align__(16) unsigned char lds_raw[];
  _Float16* wfh = (_Float16*)lds_raw;                       // [TQ][SH] hi
  _Float16* wfl = wfh + TQ * SH;                            // [TQ][SH] lo
  float4* dq_all = (float4*)(wfl + TQ * SH);                // [NWV][kKPmax]: the query's (D, m)
  float* infl_all = (float*)(dq_all + NWV * kKPmax);        // [NWV][64][kSlot]: staged influences
  int* ids_all = (int*)(infl_all + NWV * 64 * kSlot);       // [NWV][64]
  int* lcnt = ids_all + NWV * 64;                           // [TQ]

  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int p16 = lane & 15, j4 = lane >> 4;
  float4* dq = dq_all + wave * kKPmax;
  float* infl = infl_all + wave * 64 * kSlot;
  int* ids = ids_all + wave * 64;

  // operand scales of phase 2 (split_mma.h): |wf| <= 2 kmax max|x|, the weights were scaled by the same partials
  float sa, unscale;
  {
    float* shf = reinterpret_cast<float*>(lds_raw);
    const int ka = pow2_exp_for(block_absmax(x_parts, shf, n_xparts) * (2.f * (float)kmax));
    const int kb = pow2_exp_for(block_absmax(w_parts, shf, n_wparts));
    __syncthreads();
    sa = pow2f(ka);
    unscale = pow2f(-ka - kb);
  }

  const int NT = cout >> 4;
  const int mt = wave & 1, ntb = wave >> 1;
  const int half = HALF ? lane >> 5 : 0;
  const int cl = lane & (CC - 1);
  unsigned short* wfh_u = reinterpret_cast<unsigned short*>(wfh);
  unsigned short* wfl_u = reinterpret_cast<unsigned short*>(wfl);

  const int ntiles = (nq + TQ - 1) / TQ;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int q0 = tile * TQ;
    f32x4 acc2[NTW];
#pragma unroll
    for (int t = 0; t < NTW; ++t) acc2[t] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // the first 64 columns of the wave's QPW rows, loaded together and kept over the channel chunks; rows past the
    // end (the last tile) are not live: they stage nothing and leave zero rows in the tile
    KpNeighbour first[QPW];
    float qx[QPW], qy[QPW], qz[QPW];
#pragma unroll
    for (int qi = 0; qi < QPW; ++qi) {
      const int n = q0 + wave * QPW + qi;
      const size_t nc = (size_t)min(n, nq - 1);
      qx[qi] = q_xyz[3 * nc];
      qy[qi] = q_xyz[3 * nc + 1];
      qz[qi] = q_xyz[3 * nc + 2];
      first[qi] = load_neighbour(nbr + nc * nbr_stride, lane, kmax, n < nq, s_xyz, ns, qx[qi], qy[qi], qz[qi], flag);
    }

    for (int c0 = 0; c0 < cin; c0 += CC) {
      // ------------------------------ phase 1 --------------------------------
#pragma unroll
      for (int qi = 0; qi < QPW; ++qi) {
        const int ql = wave * QPW + qi;
        const int n = q0 + ql;
        const size_t nc = (size_t)min(n, nq - 1);
        float acc[kKPmax];
#pragma unroll
        for (int p = 0; p < kKPmax; ++p) acc[p] = 0.f;
        int cnt = 0;
        form_query(a, nc, lane, dq);
        {
          int nv = stage_deform(first[qi], a, dq, infl, ids, lane, cnt);
          walk_neighbours<SPR_KP_LINEAR, SPR_KP_SUM, HALF>(x + c0 + cl, true, cin, nv, infl, ids, half, acc);
          const int* row = nbr + nc * nbr_stride;
          for (int kb = 64; kb < kmax; kb += 64) {   // wider rows: 64 more columns at a time
            const KpNeighbour more = load_neighbour(row, kb + lane, kmax, n < nq, s_xyz, ns, qx[qi], qy[qi], qz[qi], flag);
            nv = stage_deform(more, a, dq, infl, ids, lane, cnt);
            walk_neighbours<SPR_KP_LINEAR, SPR_KP_SUM, HALF>(x + c0 + cl, true, cin, nv, infl, ids, half, acc);
          }
          if (HALF) {
#pragma unroll
            for (int p = 0; p < kKP; ++p) acc[p] += __shfl_xor(acc[p], 32, 64);
          }
        }
        if (half == 0) {
#pragma unroll
          for (int p = 0; p < kKP; p += 2) {
            unsigned int hu, lu;
            const float m0 = dq[p].w, m1 = p + 1 < kKP ? dq[p + 1].w : 0.f;
            split_pk_s(acc[p] * m0, acc[p + 1] * m1, sa, hu, lu);
            wfh_u[ql * SH + p * CC + cl] = (unsigned short)(hu & 0xffffu);
            wfl_u[ql * SH + p * CC + cl] = (unsigned short)(lu & 0xffffu);
            if (p + 1 < kKP) {
              wfh_u[ql * SH + (p + 1) * CC + cl] = (unsigned short)(hu >> 16);
              wfl_u[ql * SH + (p + 1) * CC + cl] = (unsigned short)(lu >> 16);
            }
          }
        }
        if (c0 == 0 && lane == 0) lcnt[ql] = cnt;
      }
      __syncthreads();
      // ------------------------------ phase 2 --------------------------------
      {
        const _Float16* ah_row = wfh + (mt * 16 + p16) * SH + 8 * j4;
        const _Float16* al_row = wfl + (mt * 16 + p16) * SH + 8 * j4;
        // fragment-order planes (k_w_prep, kpconv.hip): 512 halves per (chunk, n-tile, k-step)
        const size_t wofs = (size_t)(c0 / CC) * NT * KS * 512 + lane * 8;
        static_assert(KS % 5 == 0, "k-steps per chunk");
#pragma unroll 5
        for (int ks = 0; ks < KS; ++ks) {   // the weight fragments of five k-steps are requested together
          const f16x8 ah = *reinterpret_cast<const f16x8*>(ah_row + 32 * ks);
          const f16x8 al = *reinterpret_cast<const f16x8*>(al_row + 32 * ks);
#pragma unroll
          for (int t = 0; t < NTW; ++t) {
            const int nt = ntb + 4 * t;
            if (nt < NT) {   // wave uniform
              const size_t g = wofs + ((size_t)nt * KS + ks) * 512;
              const f16x8 bh = *reinterpret_cast<const f16x8*>(Wh + g);
              const f16x8 bl = *reinterpret_cast<const f16x8*>(Wl + g);
              acc2[t] = mma3_16(ah, al, bh, bl, acc2[t]);
            }
          }
        }
      }
      __syncthreads();
    }
    // ------------------------------ epilogue ---------------------------------
    // C layout: row (query) = 16 mt + 4 j4 + r, column (channel) = 16 nt + p16
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int ql = mt * 16 + acc_row16(r, j4);
      const int n = q0 + ql;
      if (n < nq) {
        const float inv = unscale / (float)max(lcnt[ql], 1);   // unscale: exact power of two
#pragma unroll
        for (int t = 0; t < NTW; ++t) {
          const int nt = ntb + 4 * t;
          if (nt < NT) out[(size_t)n * cout + nt * 16 + p16] = acc2[t][r] * inv;
        }
      }
    }
    __syncthreads();   // the next tile rewrites lcnt
  }
}

template <int CC>
int launch_deform_tile(const float* q_xyz, int nq, const float* s_xyz, int ns, const int* nbr, int nbr_stride, int kmax,
                       const float* x, int cin, const _Float16* Wh, const _Float16* Wl, int cout, const DeformArgs& a,
                       const unsigned char* flag, const float* x_parts, const float* w_parts, int n_xparts, int n_wparts,
                       float* out, hipStream_t stream) {
  const size_t lds = deform_lds_bytes(CC);
  auto kern = k_kpconv_deform_tile<CC>;
  if (int rc = ensure_dyn_lds((const void*)kern, 160 * 1024)) return rc;
  const int per_cu = (int)((160 * 1024) / lds);   // LDS-limited residency: 1 at 64-channel chunks
  const int ntiles = cdiv(nq, kTQ);
  const int cap = device_cu_count() * (per_cu > 0 ? per_cu : 1);
  hipLaunchKernelGGL(kern, dim3(ntiles < cap ? ntiles : cap), dim3(64 * kWaves), lds, stream, q_xyz, nq, s_xyz, ns, nbr,
                     nbr_stride, kmax, x, cin, Wh, Wl, cout, a, flag, x_parts, w_parts, n_xparts, n_wparts, out);
  SPR_LAUNCH_CHECK();
  return 0;
}

// the deformed kernel points and modulations of query n in registers (one-thread kernels)
struct QueryKernel {
  float x[kKPmax], y[kKPmax], z[kKPmax], m[kKPmax];
};
__device__ __forceinline__ void form_query_regs(const DeformArgs& a, size_t n, QueryKernel& k) {
  const float* o = a.of + n * a.of_stride;
#pragma unroll
  for (int p = 0; p < kKPmax; ++p) {
    k.x[p] = k.y[p] = k.z[p] = 0.f;
    k.m[p] = 1.f;
    if (p < a.n_kp) {
      k.x[p] = a.kpts[3 * p] + a.extent * o[3 * p];
      k.y[p] = a.kpts[3 * p + 1] + a.extent * o[3 * p + 1];
      k.z[p] = a.kpts[3 * p + 2] + a.extent * o[3 * p + 2];
      if (a.modulated) k.m[p] = 2.f / (1.f + expf(-o[3 * a.n_kp + p]));
    }
  }
}

// ---------------------------------------------------------------------------
// One thread per (query, output channel): every shape.
__global__ __launch_bounds__(256) void k_kpconv_deform_simple(const float* __restrict__ q_xyz, int nq, const float* __restrict__ s_xyz, int ns,
                                       const int* __restrict__ nbr, int nbr_stride, int kmax,
                                       const float* __restrict__ x, int cin, const float* __restrict__ W, int cout,
                                       DeformArgs a, const unsigned char* __restrict__ flag, float* __restrict__ out) {
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (long)nq * cout) return;
  const int n = (int)(gid / cout), o = (int)(gid % cout);
  const float qx = q_xyz[3 * (size_t)n], qy = q_xyz[3 * (size_t)n + 1], qz = q_xyz[3 * (size_t)n + 2];
  QueryKernel qk;
  form_query_regs(a, (size_t)n, qk);
  float acc[kKPmax];
#pragma unroll
  for (int p = 0; p < kKPmax; ++p) acc[p] = 0.f;
  int cnt = 0;
  for (int k = 0; k < kmax; ++k) {
    const int idx = nbr[(size_t)n * nbr_stride + k];
    if (idx < 0 || idx >= ns) continue;
    const float rx = s_xyz[3 * (size_t)idx] - qx, ry = s_xyz[3 * (size_t)idx + 1] - qy,
                rz = s_xyz[3 * (size_t)idx + 2] - qz;
    float w[kKPmax];
    bool keep = false;
#pragma unroll
    for (int p = 0; p < kKPmax; ++p) {
      w[p] = 0.f;
      if (p < a.n_kp) {
        const float dx = rx - qk.x[p], dy = ry - qk.y[p], dz = rz - qk.z[p];
        const float d2 = dx * dx + dy * dy + dz * dz;
        w[p] = influence_of<SPR_KP_LINEAR>(d2, a.inv_extent, 0.f);
        keep |= d2 < a.e2;
      }
    }
    if (!keep) continue;
    cnt += flag[idx];
#pragma unroll
    for (int p = 0; p < kKPmax; ++p) {
      if (p < a.n_kp && w[p] != 0.f) {
        float d = 0.f;
        for (int c = 0; c < cin; ++c) d += x[(size_t)idx * cin + c] * W[((size_t)p * cin + c) * cout + o];
        acc[p] += w[p] * d;
      }
    }
  }
  float sum = 0.f;
#pragma unroll
  for (int p = 0; p < kKPmax; ++p) sum += qk.m[p] * acc[p];
  out[(size_t)n * cout + o] = sum / (float)max(cnt, 1);
}

// min_d2[n, p] = min_k d2[n, k, p]; a shadow entry is the reference's far point.  One thread per (query, kernel point).
__global__ void k_kpconv_deform_min_d2(const float* __restrict__ q_xyz, int nq, const float* __restrict__ s_xyz, int ns,
                                       const int* __restrict__ nbr, int nbr_stride, int kmax, DeformArgs a,
                                       float* __restrict__ min_d2) {
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (long)nq * a.n_kp) return;
  const size_t n = (size_t)(gid / a.n_kp);
  const int p = (int)(gid % a.n_kp);
  const float* o = a.of + n * a.of_stride;
  const float Dx = a.kpts[3 * p] + a.extent * o[3 * p], Dy = a.kpts[3 * p + 1] + a.extent * o[3 * p + 1],
              Dz = a.kpts[3 * p + 2] + a.extent * o[3 * p + 2];
  const float qx = q_xyz[3 * n], qy = q_xyz[3 * n + 1], qz = q_xyz[3 * n + 2];
  float best = __builtin_inff();
  for (int k = 0; k < kmax; ++k) {
    const int idx = nbr[n * nbr_stride + k];
    const bool ok = idx >= 0 && idx < ns;
    const size_t sid = ok ? (size_t)idx : 0;
    const float sx = ok ? s_xyz[3 * sid] : kFarPoint, sy = ok ? s_xyz[3 * sid + 1] : kFarPoint,
                sz = ok ? s_xyz[3 * sid + 2] : kFarPoint;
    const float dx = (sx - qx) - Dx, dy = (sy - qy) - Dy, dz = (sz - qz) - Dz;
    best = fminf(best, dx * dx + dy * dy + dz * dz);
  }
  min_d2[n * a.n_kp + p] = best;
}

// ---------------------------------------------------------------------------
// Backward helpers, one wave per query (four per workgroup), phase 1's staging.
//   DX = false: wf[n, p * cin + c] = sum_k h[n,k,p] x[idx[n,k], c]  (unmodulated, un-normalised),  cnt[n] = max(1, count)
//   DX = true : dx[idx[n,k], c] += sum_p h[n,k,p] m[n,p] dwfm[n, p * cin + c]  into the fixed-point sums
template <bool DX>
__global__ __launch_bounds__(256) void k_kpconv_deform_aux(const float* __restrict__ q_xyz, int nq,
                                                           const float* __restrict__ s_xyz, int ns,
                                                           const int* __restrict__ nbr, int nbr_stride, int kmax,
                                                           const float* __restrict__ x, int cin, DeformArgs a,
                                                           const float* __restrict__ dwfm, float* __restrict__ wf,
                                                           float* __restrict__ cnt_out,
                                                           const unsigned char* __restrict__ flag,
                                                           const float* __restrict__ parts, float fx_factor,
                                                           unsigned long long* __restrict__ dx_acc) {
  __shared__ __align__(16) float infl_s[4][64 * kSlot];
  __shared__ int ids_s[4][64];
  __shared__ float4 dq_s[4][kKPmax];
  int fx = 0;
  if (DX) {   // |sum_p h m dwfm| <= fx_factor max |dwfm|: h <= 1, m < 2
    __shared__ float sh[17];
    fx = fx_exp(parts, sh, fx_factor);
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + wave;
  if (n >= nq) return;   // whole wave
  float* infl = infl_s[wave];
  int* ids = ids_s[wave];
  float4* dq = dq_s[wave];
  form_query(a, (size_t)n, lane, dq);
  const float qx = q_xyz[3 * (size_t)n], qy = q_xyz[3 * (size_t)n + 1], qz = q_xyz[3 * (size_t)n + 2];
  const int* row = nbr + (size_t)n * nbr_stride;
  const int nchunk = (cin + 63) / 64;
  int cnt = 0;
  for (int kb = 0; kb < kmax; kb += 64) {
    const KpNeighbour nb = load_neighbour(row, kb + lane, kmax, true, s_xyz, ns, qx, qy, qz, DX ? nullptr : flag);
    const int nv = stage_deform(nb, a, dq, infl, ids, lane, cnt);
    for (int c0 = 0; c0 < nchunk; ++c0) {
      const int c = c0 * 64 + lane;
      const bool cok = c < cin;
      float acc[kKPmax];
#pragma unroll
      for (int p = 0; p < kKPmax; ++p) acc[p] = 0.f;
      if constexpr (!DX) {
        walk_neighbours<SPR_KP_LINEAR, SPR_KP_SUM, false>(x + (cok ? c : 0), cok, cin, nv, infl, ids, 0, acc);
        // (the first pass stores; later passes of a wider row add to what it wrote)
        if (cok) {
#pragma unroll
          for (int p = 0; p < kKPmax; ++p)
            if (p < a.n_kp) {
              float* dst = wf + ((size_t)n * a.n_kp + p) * cin + c;
              *dst = kb == 0 ? acc[p] : *dst + acc[p];
            }
        }
      } else {
#pragma unroll
        for (int p = 0; p < kKPmax; ++p)
          acc[p] = (cok && p < a.n_kp) ? dwfm[((size_t)n * a.n_kp + p) * cin + c] * dq[p].w : 0.f;
        for (int k = 0; k < nv; ++k) {
          const float* iw = infl + k * kSlot;
          float v = 0.f;
#pragma unroll
          for (int p4 = 0; p4 < kKPmax / 4; ++p4) {
            const float4 w4 = *reinterpret_cast<const float4*>(iw + 4 * p4);
            v += w4.x * acc[4 * p4];
            v += w4.y * acc[4 * p4 + 1];
            v += w4.z * acc[4 * p4 + 2];
            v += w4.w * acc[4 * p4 + 3];
          }
          if (cok && v != 0.f) fx_add(dx_acc + (size_t)ids[k] * cin + c, v, fx);
        }
      }
    }
  }
  if (!DX && lane == 0) cnt_out[n] = (float)max(cnt, 1);
}

// d of [nq, (3 + modulated) n_kp], every element written.  One wave per query, lane = neighbour.
__global__ __launch_bounds__(256) void k_kpconv_deform_offsets(const float* __restrict__ q_xyz, int nq,
                                                               const float* __restrict__ s_xyz, int ns,
                                                               const int* __restrict__ nbr, int nbr_stride, int kmax,
                                                               const float* __restrict__ x, int cin, DeformArgs a,
                                                               const float* __restrict__ dwfm,
                                                               float* __restrict__ d_of) {
  __shared__ __align__(16) float g_s[4][64 * kKPmax];   // dwfm[n, :, c0 .. c0 + 64) as [channel][kernel point]
  __shared__ float4 dq_s[4][kKPmax];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + wave;
  if (n >= nq) return;   // whole wave
  float* gs = g_s[wave];
  float4* dq = dq_s[wave];
  form_query(a, (size_t)n, lane, dq);
  const float qx = q_xyz[3 * (size_t)n], qy = q_xyz[3 * (size_t)n + 1], qz = q_xyz[3 * (size_t)n + 2];
  const int* row = nbr + (size_t)n * nbr_stride;
  const float* grow = dwfm + (size_t)n * a.n_kp * cin;
  // the lane's partial sums over its neighbours (columns lane, lane + 64, ...): d D (unscaled) and d m
  float sx[kKPmax], sy[kKPmax], sz[kKPmax], sm[kKPmax];
#pragma unroll
  for (int p = 0; p < kKPmax; ++p) sx[p] = sy[p] = sz[p] = sm[p] = 0.f;

  for (int kb = 0; kb < kmax; kb += 64) {
    const KpNeighbour nb = load_neighbour(row, kb + lane, kmax, true, s_xyz, ns, qx, qy, qz, nullptr);
    bool keep = false;
    if (nb.id >= 0) {
#pragma unroll
      for (int p = 0; p < kKPmax; ++p) {
        if (p < a.n_kp) {
          const float4 d = dq[p];
          const float dx = nb.px - d.x, dy = nb.py - d.y, dz = nb.pz - d.z;
          keep |= dx * dx + dy * dy + dz * dz < a.e2;
        }
      }
    }
    if (__ballot(keep) == 0ull) continue;   // wave uniform
    float g[kKPmax];                        // g[p] = sum_c dwfm[n,p,c] x[id,c]
#pragma unroll
    for (int p = 0; p < kKPmax; ++p) g[p] = 0.f;
    for (int c0 = 0; c0 < cin; c0 += 64) {
      const bool cok = c0 + lane < cin;
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int p4 = 0; p4 < kKPmax / 4; ++p4) {
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
          v[j] = (cok && 4 * p4 + j < a.n_kp) ? grow[(size_t)(4 * p4 + j) * cin + c0 + lane] : 0.f;
        *reinterpret_cast<float4*>(gs + lane * kKPmax + 4 * p4) = make_float4(v[0], v[1], v[2], v[3]);
      }
      __builtin_amdgcn_wave_barrier();
      if (keep) {
        const float* xr = x + (size_t)nb.id * cin + c0;
        const int nc = min(64, cin - c0);
        for (int c = 0; c < nc; ++c) {
          const float xv = xr[c];
#pragma unroll
          for (int p4 = 0; p4 < kKPmax / 4; ++p4) {
            const float4 w4 = *reinterpret_cast<const float4*>(gs + c * kKPmax + 4 * p4);
            g[4 * p4] += w4.x * xv;
            g[4 * p4 + 1] += w4.y * xv;
            g[4 * p4 + 2] += w4.z * xv;
            g[4 * p4 + 3] += w4.w * xv;
          }
        }
      }
    }
    if (keep) {
#pragma unroll
      for (int p = 0; p < kKPmax; ++p) {
        if (p < a.n_kp) {
          const float4 d = dq[p];
          const float dx = nb.px - d.x, dy = nb.py - d.y, dz = nb.pz - d.z;
          const float dist = sqrtf(dx * dx + dy * dy + dz * dz);
          sm[p] += fmaxf(0.f, 1.f - dist * a.inv_extent) * g[p];
          if (dist > 0.f && dist < a.extent) {   // dist == 0: no contribution (see the head of the file)
            const float coef = g[p] / (dist * a.extent);
            sx[p] += coef * dx;
            sy[p] += coef * dy;
            sz[p] += coef * dz;
          }
        }
      }
    }
  }
  float* o = d_of + (size_t)n * ((a.modulated ? 4 : 3) * a.n_kp);
#pragma unroll
  for (int p = 0; p < kKPmax; ++p) {
    if (p < a.n_kp) {   // wave uniform
      const float tx = wave_sum(sx[p]), ty = wave_sum(sy[p]), tz = wave_sum(sz[p]), tm = wave_sum(sm[p]);
      if (lane == p) {
        const float m = dq[p].w, em = a.extent * m;
        o[3 * p] = em * tx;
        o[3 * p + 1] = em * ty;
        o[3 * p + 2] = em * tz;
        if (a.modulated) o[3 * a.n_kp + p] = tm * (m * (1.f - 0.5f * m));   // 2 s (1 - s) with m = 2 s
      }
    }
  }
}

// the workspace of the forward: the flags of launch_rowflag, then what the tile kernel needs
struct DeformWs {
  unsigned char* flag;
  float4* sxf;             // launch_rowflag's support records (unused here; it writes them)
  int* tile_ctr;
  unsigned char* wplanes;  // spr_kpconv_wplanes_bytes(cin, cout) when the shape has planes
  float *x_parts, *w_parts;
};
inline bool plane_shape(int cin, int cout) { return cin > 0 && cin % 32 == 0 && cout > 0 && cout % 32 == 0 && cout <= 256; }
DeformWs deform_layout(Workspace& w, int nq, int ns, int cin, int cout) {
  (void)nq;
  const size_t n = (size_t)(ns > 0 ? ns : 1);
  DeformWs l;
  l.flag = w.take<unsigned char>(n);
  l.sxf = w.take<float4>(n + 1);
  l.tile_ctr = w.take<int>(64);
  l.wplanes = w.take<unsigned char>(plane_shape(cin, cout) ? spr_kpconv_wplanes_bytes(cin, cout) : 0);
  l.x_parts = w.take<float>(kAmaxParts);
  l.w_parts = w.take<float>(kAmaxParts);
  return l;
}
struct DeformFlagWs {
  unsigned char* flag;
  float4* sxf;
  int* tile_ctr;
};
DeformFlagWs deform_flag_layout(Workspace& w, int ns) {
  const size_t n = (size_t)(ns > 0 ? ns : 1);
  DeformFlagWs l;
  l.flag = w.take<unsigned char>(n);
  l.sxf = w.take<float4>(n + 1);
  l.tile_ctr = w.take<int>(64);
  return l;
}

// the arguments every entry point shares
int check_common(const char* what, int nq, int ns, int nbr_stride, int kmax, int cin, int n_kp, float kp_extent,
                 const float* offset_features, int of_stride, int modulated) {
  SPR_REQUIRE(nq > 0 && ns > 0, "%s: empty input", what);
  SPR_REQUIRE(kmax >= 1 && kmax <= nbr_stride, "%s: bad kmax=%d stride=%d", what, kmax, nbr_stride);
  SPR_REQUIRE(cin >= 1 && n_kp >= 1 && n_kp <= kKPmax, "%s: bad dims (at most %d kernel points)", what, kKPmax);
  SPR_REQUIRE(kp_extent > 0.f, "%s: KP_extent must be > 0", what);
  SPR_REQUIRE(modulated == 0 || modulated == 1, "%s: modulated is 0 or 1", what);
  SPR_REQUIRE(offset_features != nullptr && of_stride >= (3 + modulated) * n_kp,
              "%s: offset features need %d columns, row stride %d", what, (3 + modulated) * n_kp, of_stride);
  return 0;
}
DeformArgs deform_args(const float* kernel_points, int n_kp, float kp_extent, const float* offset_features,
                       int of_stride, int modulated) {
  // e^2 as the reference forms it: a Python float, compared with float32 distances
  return DeformArgs{kernel_points, n_kp, kp_extent, 1.0f / kp_extent, (float)((double)kp_extent * (double)kp_extent),
                    offset_features, of_stride, modulated};
}

}  // namespace
}  // namespace spr

using namespace spr;

extern "C" size_t spr_kpconv_deform_workspace_size(int nq, int ns, int cin, int cout) {
  return measure(deform_layout, nq, ns, cin, cout);
}

extern "C" int spr_kpconv_deform_fwd(const float* q_xyz, int nq, const float* s_xyz, int ns, const int* nbr,
                                     int nbr_stride, int kmax, const float* x, int cin, const float* weights, int cout,
                                     const float* kernel_points, int n_kp, float kp_extent,
                                     const float* offset_features, int of_stride, int modulated, float* out,
                                     float* min_d2, int impl, const float* x_range, int x_range_n,
                                     const float* w_range, int w_range_n, const void* wplanes, void* ws,
                                     size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (int rc = check_common("kpconv_deform", nq, ns, nbr_stride, kmax, cin, n_kp, kp_extent, offset_features, of_stride,
                            modulated))
    return rc;
  SPR_REQUIRE((x_range == nullptr || x_range_n >= 1) && (w_range == nullptr || w_range_n >= 1),
              "kpconv_deform: a range needs a count");
  SPR_REQUIRE(cout >= 1, "kpconv_deform: bad dims");
  SPR_REQUIRE(impl == 0 || impl == 1, "kpconv_deform: impl is 0 or 1");
  Workspace w(ws, ws_bytes);
  const DeformWs l = deform_layout(w, nq, ns, cin, cout);
  SPR_REQUIRE(ws != nullptr && w.ok(), "kpconv_deform: workspace too small");
  SPR_REQUIRE(wplanes == nullptr || w_range != nullptr,
              "kpconv_deform: prepared weight planes come with the range they were scaled by");
  const DeformArgs a = deform_args(kernel_points, n_kp, kp_extent, offset_features, of_stride, modulated);

  launch_rowflag(x, s_xyz, ns, cin, l.flag, l.sxf, l.tile_ctr, stream);
  SPR_LAUNCH_CHECK();
  if (min_d2 != nullptr) {
    hipLaunchKernelGGL(k_kpconv_deform_min_d2, dim3(cdiv((long)nq * n_kp, 256)), dim3(256), 0, stream, q_xyz, nq, s_xyz,
                       ns, nbr, nbr_stride, kmax, a, min_d2);
    SPR_LAUNCH_CHECK();
  }

  if (impl == 0 && n_kp == kKP && plane_shape(cin, cout)) {
    const int ktot = n_kp * cin;
    const float* xp = x_range != nullptr ? x_range : l.x_parts;
    const float* wp = w_range != nullptr ? w_range : l.w_parts;
    const int n_xp = x_range != nullptr ? x_range_n : kAmaxParts, n_wp = w_range != nullptr ? w_range_n : kAmaxParts;
    if (x_range == nullptr)
      if (int rc = launch_absmax(x, ns, cin, cin, l.x_parts, stream)) return rc;
    if (w_range == nullptr)
      if (int rc = launch_absmax(weights, ktot, cout, cout, l.w_parts, stream)) return rc;
    const void* planes = wplanes;
    if (planes == nullptr) {
      if (int rc = spr_kpconv_prep_weights(weights, n_kp, cin, cout, wp, n_wp, l.wplanes,
                                           spr_kpconv_wplanes_bytes(cin, cout), stream_))
        return rc;
      planes = l.wplanes;
    }
    // the planes' own carve (spr_kpconv_prep_weights): hi, then lo, room for 32 kernel points each
    Workspace pv(const_cast<void*>(planes), SIZE_MAX);
    const size_t n_half = (size_t)32 * cin * cout;
    const _Float16* wh = pv.take<_Float16>(n_half);
    const _Float16* wl = pv.take<_Float16>(n_half);
    return cin % 64 == 0
               ? launch_deform_tile<64>(q_xyz, nq, s_xyz, ns, nbr, nbr_stride, kmax, x, cin, wh, wl, cout, a,
                                        (const unsigned char*)l.flag, xp, wp, n_xp, n_wp, out, stream)
               : launch_deform_tile<32>(q_xyz, nq, s_xyz, ns, nbr, nbr_stride, kmax, x, cin, wh, wl, cout, a,
                                        (const unsigned char*)l.flag, xp, wp, n_xp, n_wp, out, stream);
  }
  const long total = (long)nq * cout;
  hipLaunchKernelGGL(k_kpconv_deform_simple, dim3(cdiv(total, 256)), dim3(256), 0, stream, q_xyz, nq, s_xyz, ns, nbr,
                     nbr_stride, kmax, x, cin, weights, cout, a, (const unsigned char*)l.flag, out);
  SPR_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t spr_kpconv_deform_weighted_features_workspace_size(int ns) {
  return measure(deform_flag_layout, ns);
}

extern "C" int spr_kpconv_deform_weighted_features(const float* q_xyz, int nq, const float* s_xyz, int ns,
                                                   const int* nbr, int nbr_stride, int kmax, const float* x, int cin,
                                                   const float* kernel_points, int n_kp, float kp_extent,
                                                   const float* offset_features, int of_stride, float* wf, float* cnt,
                                                   void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (int rc = check_common("kpconv_deform_weighted_features", nq, ns, nbr_stride, kmax, cin, n_kp, kp_extent,
                            offset_features, of_stride, 0))
    return rc;
  Workspace w(ws, ws_bytes);
  const DeformFlagWs l = deform_flag_layout(w, ns);
  SPR_REQUIRE(ws != nullptr && w.ok(), "kpconv_deform_weighted_features: workspace too small");
  launch_rowflag(x, s_xyz, ns, cin, l.flag, l.sxf, l.tile_ctr, stream);
  hipLaunchKernelGGL((k_kpconv_deform_aux<false>), dim3(cdiv(nq, 4)), dim3(256), 0, stream, q_xyz, nq, s_xyz, ns, nbr,
                     nbr_stride, kmax, x, cin, deform_args(kernel_points, n_kp, kp_extent, offset_features, of_stride, 0),
                     (const float*)nullptr, wf, cnt, (const unsigned char*)l.flag, (const float*)nullptr, 0.f,
                     (unsigned long long*)nullptr);
  SPR_LAUNCH_CHECK();
  return 0;
}

extern "C" int spr_kpconv_deform_bwd_dx(const float* q_xyz, int nq, const float* s_xyz, int ns, const int* nbr,
                                        int nbr_stride, int kmax, int cin, const float* kernel_points, int n_kp,
                                        float kp_extent, const float* offset_features, int of_stride, int modulated,
                                        const float* dwfm, const float* dwfm_range, int dwfm_range_n, float* dx,
                                        void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (int rc = check_common("kpconv_deform_bwd_dx", nq, ns, nbr_stride, kmax, cin, n_kp, kp_extent, offset_features,
                            of_stride, modulated))
    return rc;
  SPR_REQUIRE(dwfm_range == nullptr || dwfm_range_n >= 1, "kpconv_deform_bwd_dx: a range needs a count");
  FxScratch f;
  if (int rc = fx_scratch(ws, ws_bytes, ns, cin, stream, &f)) return rc;
  if (dwfm_range != nullptr) {
    hipLaunchKernelGGL(k_range_to_parts, dim3(1), dim3(256), 0, stream, dwfm_range, dwfm_range_n, f.parts);
  } else if (int rc = launch_absmax(dwfm, nq, n_kp * cin, n_kp * cin, f.parts, stream)) {
    return rc;
  }
  const float factor = (float)((modulated ? 2 : 1) * n_kp);
  hipLaunchKernelGGL((k_kpconv_deform_aux<true>), dim3(cdiv(nq, 4)), dim3(256), 0, stream, q_xyz, nq, s_xyz, ns, nbr,
                     nbr_stride, kmax, (const float*)nullptr, cin,
                     deform_args(kernel_points, n_kp, kp_extent, offset_features, of_stride, modulated), dwfm,
                     (float*)nullptr, (float*)nullptr, (const unsigned char*)nullptr, (const float*)f.parts, factor,
                     f.acc);
  hipLaunchKernelGGL(k_fx_to_float, dim3(cdiv((long)ns * cin, 256)), dim3(256), 0, stream, f.acc, (long)ns * cin,
                     f.parts, factor, dx);
  SPR_LAUNCH_CHECK();
  return 0;
}

extern "C" int spr_kpconv_deform_bwd_offsets(const float* q_xyz, int nq, const float* s_xyz, int ns, const int* nbr,
                                             int nbr_stride, int kmax, const float* x, int cin,
                                             const float* kernel_points, int n_kp, float kp_extent,
                                             const float* offset_features, int of_stride, int modulated,
                                             const float* dwfm, float* d_offset_features, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (int rc = check_common("kpconv_deform_bwd_offsets", nq, ns, nbr_stride, kmax, cin, n_kp, kp_extent,
                            offset_features, of_stride, modulated))
    return rc;
  SPR_REQUIRE(dwfm != nullptr && d_offset_features != nullptr, "kpconv_deform_bwd_offsets: null gradient");
  hipLaunchKernelGGL(k_kpconv_deform_offsets, dim3(cdiv(nq, 4)), dim3(256), 0, stream, q_xyz, nq, s_xyz, ns, nbr,
                     nbr_stride, kmax, x, cin,
                     deform_args(kernel_points, n_kp, kp_extent, offset_features, of_stride, modulated), dwfm,
                     d_offset_features);
  SPR_LAUNCH_CHECK();
  return 0;
}
