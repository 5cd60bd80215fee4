// KPConv with the reference's other influence functions and aggregation rule (rigid kernel points) on gfx950:
// {constant, linear, gaussian} x {sum, closest}, forward and the two non-GEMM pieces of the backward.
//
// Behaviour contract: KPConv.forward, models/backbone_kpconv/kpconv_blocks.py:309-412
//     :325-329  d2[n,k,p] = |s[idx[n,k]] - q[n] - kp[p]|^2                       (float32)
//     :361-377  influence  constant: 1   linear: max(0, 1 - sqrt(d2) / extent)
//               gaussian: exp(-d2 / (2 sigma^2 + 1e-9)), sigma = 0.3 extent      (no cut-off)
//     :380-382  closest: the influence is kept at p = argmin_p d2 only (lowest p on a tie, torch.argmin)
//     :388-406  wf[n,p,:] = sum_k w[n,k,p] x[idx[n,k],:];  out[n,:] = sum_p wf[n,p,:] W[p]
//     :409-412  out /= max(1, #{k : sum_c x[idx[n,k],c] > 0})
// A shadow neighbour (index outside [0, ns)) contributes nothing and is not counted: the reference's far point with
// a zero feature row gives the same in every mode.  The count comes from launch_rowflag (kpconv.hip), the flags of
// the linear / sum kernels: the summation order of the sign test is part of the result.
//
// linear / sum is a valid mode here (the cross-check against kpconv.hip); ops.kpconv never routes it here.
//
// Forward: k_kpconv_modes_tile<INFL, AGG, CC>, one workgroup of 8 waves per tile of 32 queries.
//   phase 1 (wave = 4 queries, one after the other): lane = neighbour computes the neighbour's influences (SUM: 15
//     floats; CLOSEST: the arg-min kernel point and its influence) and parks them, valid neighbours compacted, in LDS;
//     then lane = channel walks the staged neighbours, eight gathered values in flight:
//       sum       acc[p] += w[p] x           (constant: all 15 slots are the same sum -- one accumulator)
//       closest   acc[pmin] += w x           (pmin is wave uniform: the register array is indexed through M0, one
//                                             FMA, not a 15-wide contraction; CC = 32 packs two neighbours per
//                                             wave: 15 selects)
//     (the index, position and flag loads of the wave's four rows are issued together, once per tile)
//     the 15 sums of a channel leave as split-fp16 hi / lo halves in the [32 x 15 CC] tile (scale: kmax max|x|, every
//     influence is <= 1 in every mode);
//   phase 2: the tile x W[15 CC, cout] by v_mfma_f32_16x16x32_f16 triples (split_mma.h) against the fragment-order
//     planes of spr_kpconv_prep_weights; wave -> (m-tile w & 1, n-tiles (w >> 1) + 4 t); accumulators persist over
//     the channel chunks of wider inputs.
//   LDS at CC = 64: 2 x 32 x 976 halves = 122 KB tile + 8 x 64 x 16 floats = 32 KB staged influences (closest: 8 x
//     64 x 2 floats = 4 KB) + 2 KB indices = 156 KB of the CU's 160 (one workgroup per CU); CC = 32: 96 KB.  Nothing in it grows with kmax: rows wider
//     than 64 neighbours are staged 64 at a time.
// Other shapes (cin or cout no multiple of 32, cout > 256, cin == 1, n_kp != 15) and impl == 1: k_kpconv_modes_simple,
//   one thread per output element, the same mode switch.
// Backward: k_kpconv_modes_aux<INFL, AGG, DX>, one wave per query with phase 1's staging: wf + count, or the scatter
//   of influence x d wf into 64-bit fixed-point sums (fx_scatter.h: the bits do not depend on the arrival order).
#include "spr_common.h"
#include "fx_scatter.h"
#include "split_mma.h"
#include "kpconv_walk.h"

namespace spr {
namespace {

constexpr int kKP = 15;       // kernel points of the tile kernel
constexpr int kKPmax = 16;    // kernel points of the one-wave-per-query kernels
static_assert(kKPmax == kWalkKP, "walk_neighbours' accumulators");

struct KpModeArgs {
  const float* kpts;
  int n_kp;
  float inv_extent, gauss_den;
};

// Lane = one neighbour of a query's row (load_neighbour, kpconv_walk.h).  stage_neighbours: influences -> LDS, valid
// neighbours compacted in row order (the walk that follows has no holes and sums in ascending position); cnt +=
// neighbours whose flag is set; returns the number staged (wave uniform).  Two wave barriers: the previous walk's
// reads, this staging's writes.
template <int INFL, int AGG>
__device__ __forceinline__ int stage_neighbours(const KpNeighbour& nb, const KpModeArgs& a, float* __restrict__ infl,
                                                int* __restrict__ ids, int lane, int& cnt) {
  const int id = nb.id;
  const bool ok = id >= 0;
  float w[kKPmax];
  int pmin = 0;
  if (ok) {
    const float px = nb.px, py = nb.py, pz = nb.pz;
    float best = 0.f;
#pragma unroll
    for (int p = 0; p < kKPmax; ++p) {
      w[p] = 0.f;
      if (p < a.n_kp) {
        const float dx = px - a.kpts[3 * p], dy = py - a.kpts[3 * p + 1], dz = pz - a.kpts[3 * p + 2];
        const float d2 = dx * dx + dy * dy + dz * dz;
        if constexpr (AGG == SPR_KP_SUM) {
          w[p] = influence_of<INFL>(d2, a.inv_extent, a.gauss_den);
        } else if (p == 0 || d2 < best) {   // strict: the lowest p wins a tie
          best = d2;
          pmin = p;
        }
      }
    }
    if constexpr (AGG == SPR_KP_CLOSEST) w[0] = influence_of<INFL>(best, a.inv_extent, a.gauss_den);
  }
  const unsigned long long m = __ballot(ok);
  cnt += __popcll(__ballot(ok && nb.pos != 0));
  const int slot = __popcll(m & ((1ull << lane) - 1ull));
  constexpr int SLOT = slot_floats(AGG);
  __builtin_amdgcn_wave_barrier();
  if (ok) {
    ids[slot] = id;
    if constexpr (AGG == SPR_KP_CLOSEST) {
      *reinterpret_cast<float2*>(infl + slot * SLOT) = make_float2(w[0], __int_as_float(pmin));
    } else if constexpr (INFL != SPR_KP_CONSTANT) {
#pragma unroll
      for (int p4 = 0; p4 < kKPmax / 4; ++p4)
        *reinterpret_cast<float4*>(infl + slot * SLOT + 4 * p4) =
            make_float4(w[4 * p4], w[4 * p4 + 1], w[4 * p4 + 2], w[4 * p4 + 3]);
    }
  }
  __builtin_amdgcn_wave_barrier();
  return __popcll(m);
}

#define SPR_KP_CASES(C) C(0) C(1) C(2) C(3) C(4) C(5) C(6) C(7) C(8) C(9) C(10) C(11) C(12) C(13) C(14) C(15)

// (the lane = channel walk over the staged neighbours: walk_neighbours, kpconv_walk.h)

// ---------------------------------------------------------------------------
// Fused tile kernel (see the head of the file).
constexpr int kModesTQ = 32, kModesWaves = 8;

// floats of a wave's phase-1 scratch: the staged influences of 64 neighbours
constexpr int wave_scratch_floats(int agg) { return 64 * slot_floats(agg); }
static inline size_t modes_lds_bytes(int cc, int agg) {
  return 2 * sizeof(_Float16) * (size_t)kModesTQ * (kKP * cc + 16) +
         sizeof(float) * kModesWaves * wave_scratch_floats(agg) + sizeof(int) * kModesWaves * 64 + sizeof(int) * kModesTQ;
}

template <int INFL, int AGG, int CC>
__global__ __launch_bounds__(64 * kModesWaves) void k_kpconv_modes_tile(
    const float* __restrict__ q_xyz, int nq, const float* __restrict__ s_xyz, int ns, const int* __restrict__ nbr,
    int nbr_stride, int kmax, const float* __restrict__ x, int cin, const _Float16* __restrict__ Wh,
    const _Float16* __restrict__ Wl, int cout, KpModeArgs a, const unsigned char* __restrict__ flag,
    const float* __restrict__ x_parts, const float* __restrict__ w_parts, int n_xparts, int n_wparts,
    float* __restrict__ out) {
  constexpr int TQ = kModesTQ, NWV = kModesWaves, QPW = TQ / NWV;
  constexpr int KW = kKP * CC;       // phase-2 K per chunk
  constexpr int SH = KW + 16;        // LDS row stride in halves (k_kpconv_mfma's: conflict-free fragment reads)
  constexpr int KS = KW / 32;        // 32-deep k-steps per chunk
  constexpr bool HALF = CC == 32;
  constexpr bool ONE_SUM = INFL == SPR_KP_CONSTANT && AGG == SPR_KP_SUM;
  constexpr int NTW = 4;             // n-tiles per wave at most (cout <= 256)
  static_assert(CC == 32 || CC == 64, "channel chunk");
  extern __shared__ __align__(16) unsigned char lds_raw[];
  _Float16* wfh = (_Float16*)lds_raw;                       // [TQ][SH] hi
  _Float16* wfl = wfh + TQ * SH;                            // [TQ][SH] lo
  constexpr int WSCR = wave_scratch_floats(AGG);
  float* infl_all = (float*)(wfl + TQ * SH);                // [NWV][WSCR]: staged influences
  int* ids_all = (int*)(infl_all + NWV * WSCR);             // [NWV][64]
  int* lcnt = ids_all + NWV * 64;                           // [TQ]

  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int p16 = lane & 15, j4 = lane >> 4;
  float* infl = infl_all + wave * WSCR;
  int* ids = ids_all + wave * 64;

  // operand scales of phase 2 (split_mma.h): |wf| <= kmax max|x|, the weights were scaled by the same partials
  float sa, unscale;
  {
    float* shf = reinterpret_cast<float*>(lds_raw);
    const int ka = pow2_exp_for(block_absmax(x_parts, shf, n_xparts) * (float)kmax);
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

    // The first 64 columns of the wave's QPW rows: all index loads, then all position / flag loads, in flight
    // together -- two memory round trips per tile instead of two per query and channel chunk (kept over the chunks).
    // Rows past the end (the last tile) are not live: they stage nothing and leave zero rows in the tile.
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
        float acc[kKPmax];
#pragma unroll
        for (int p = 0; p < kKPmax; ++p) acc[p] = 0.f;
        int cnt = 0;
        {
          int nv = stage_neighbours<INFL, AGG>(first[qi], a, infl, ids, lane, cnt);
          walk_neighbours<INFL, AGG, HALF>(x + c0 + cl, true, cin, nv, infl, ids, half, acc);
          const int* row = nbr + (size_t)min(n, nq - 1) * nbr_stride;
          for (int kb = 64; kb < kmax; kb += 64) {   // wider rows: 64 more columns at a time
            const KpNeighbour more = load_neighbour(row, kb + lane, kmax, n < nq, s_xyz, ns, qx[qi], qy[qi], qz[qi], flag);
            nv = stage_neighbours<INFL, AGG>(more, a, infl, ids, lane, cnt);
            walk_neighbours<INFL, AGG, HALF>(x + c0 + cl, true, cin, nv, infl, ids, half, acc);
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
            split_pk_s(ONE_SUM ? acc[0] : acc[p], ONE_SUM ? acc[0] : acc[p + 1], sa, hu, lu);
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

template <int INFL, int AGG, int CC>
int launch_modes_tile(const float* q_xyz, int nq, const float* s_xyz, int ns, const int* nbr, int nbr_stride, int kmax,
                      const float* x, int cin, const _Float16* Wh, const _Float16* Wl, int cout, const KpModeArgs& a,
                      const unsigned char* flag, const float* x_parts, const float* w_parts, int n_xparts, int n_wparts,
                      float* out, hipStream_t stream) {
  const size_t lds = modes_lds_bytes(CC, AGG);
  auto kern = k_kpconv_modes_tile<INFL, AGG, CC>;
  if (int rc = ensure_dyn_lds((const void*)kern, 160 * 1024)) return rc;
  const int per_cu = (int)((160 * 1024) / lds);   // LDS-limited residency: 1 at 64-channel chunks
  const int ntiles = cdiv(nq, kModesTQ);
  const int cap = device_cu_count() * (per_cu > 0 ? per_cu : 1);
  hipLaunchKernelGGL(kern, dim3(ntiles < cap ? ntiles : cap), dim3(64 * kModesWaves), lds, stream, q_xyz, nq, s_xyz, ns,
                     nbr, nbr_stride, kmax, x, cin, Wh, Wl, cout, a, flag, x_parts, w_parts, n_xparts, n_wparts, out);
  SPR_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------
// One thread per (query, output channel): every shape, every mode.
__global__ void k_kpconv_modes_simple(const float* __restrict__ q_xyz, int nq, const float* __restrict__ s_xyz, int ns,
                                      const int* __restrict__ nbr, int nbr_stride, int kmax,
                                      const float* __restrict__ x, int cin, const float* __restrict__ W, int cout,
                                      KpModeArgs a, int infl, int agg, const unsigned char* __restrict__ flag,
                                      float* __restrict__ out) {
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (long)nq * cout) return;
  const int n = (int)(gid / cout), o = (int)(gid % cout);
  const float qx = q_xyz[3 * (size_t)n], qy = q_xyz[3 * (size_t)n + 1], qz = q_xyz[3 * (size_t)n + 2];
  auto influence = [&](float d2) {
    return infl == SPR_KP_CONSTANT ? 1.f
           : infl == SPR_KP_LINEAR ? influence_of<SPR_KP_LINEAR>(d2, a.inv_extent, a.gauss_den)
                                   : influence_of<SPR_KP_GAUSSIAN>(d2, a.inv_extent, a.gauss_den);
  };
  auto row_dot = [&](int idx, int p) {
    float d = 0.f;
    for (int c = 0; c < cin; ++c) d += x[(size_t)idx * cin + c] * W[((size_t)p * cin + c) * cout + o];
    return d;
  };
  float acc = 0.f;
  int cnt = 0;
  for (int k = 0; k < kmax; ++k) {
    const int idx = nbr[(size_t)n * nbr_stride + k];
    if (idx < 0 || idx >= ns) continue;
    cnt += flag[idx];
    const float rx = s_xyz[3 * (size_t)idx] - qx, ry = s_xyz[3 * (size_t)idx + 1] - qy,
                rz = s_xyz[3 * (size_t)idx + 2] - qz;
    float best = 0.f;
    int pmin = 0;
    for (int p = 0; p < a.n_kp; ++p) {
      const float dx = rx - a.kpts[3 * p], dy = ry - a.kpts[3 * p + 1], dz = rz - a.kpts[3 * p + 2];
      const float d2 = dx * dx + dy * dy + dz * dz;
      if (agg == SPR_KP_SUM) {
        const float w = influence(d2);
        if (w != 0.f) acc += w * row_dot(idx, p);
      } else if (p == 0 || d2 < best) {
        best = d2;
        pmin = p;
      }
    }
    if (agg == SPR_KP_CLOSEST) {
      const float w = influence(best);
      if (w != 0.f) acc += w * row_dot(idx, pmin);
    }
  }
  out[(size_t)n * cout + o] = acc / (float)max(cnt, 1);
}

// ---------------------------------------------------------------------------
// Backward helpers, one wave per query (four per workgroup).
//   DX = false: wf[n, p * cin + c] = sum_k infl[n,k,p] x[idx[n,k], c]  (un-normalised),  cnt[n] = max(1, count)
//   DX = true : dx[idx[n,k], c] += sum_p infl[n,k,p] dwf[n, p * cin + c]  into the fixed-point sums
// The influences (and the arg-min of `closest`) are constants of the backward: kernel points are not trained.
template <int INFL, int AGG, bool DX>
__global__ __launch_bounds__(256) void k_kpconv_modes_aux(const float* __restrict__ q_xyz, int nq,
                                                          const float* __restrict__ s_xyz, int ns,
                                                          const int* __restrict__ nbr, int nbr_stride, int kmax,
                                                          const float* __restrict__ x, int cin, KpModeArgs a,
                                                          const float* __restrict__ dwf, float* __restrict__ wf,
                                                          float* __restrict__ cnt_out,
                                                          const unsigned char* __restrict__ flag,
                                                          const float* __restrict__ parts,
                                                          unsigned long long* __restrict__ dx_acc) {
  __shared__ __align__(16) float infl_s[4][64 * kSlot];
  __shared__ int ids_s[4][64];
  constexpr bool ONE_SUM = INFL == SPR_KP_CONSTANT && AGG == SPR_KP_SUM;
  int fx = 0;
  if (DX) {   // |sum_p infl[p] dwf[p]| <= n_kp max |dwf|: every influence is <= 1
    __shared__ float sh[17];
    fx = fx_exp(parts, sh, (float)a.n_kp);
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + wave;
  if (n >= nq) return;   // whole wave
  float* infl = infl_s[wave];
  int* ids = ids_s[wave];
  const float qx = q_xyz[3 * (size_t)n], qy = q_xyz[3 * (size_t)n + 1], qz = q_xyz[3 * (size_t)n + 2];
  const int* row = nbr + (size_t)n * nbr_stride;
  const int nchunk = (cin + 63) / 64;
  int cnt = 0;
  for (int kb = 0; kb < kmax; kb += 64) {
    const KpNeighbour nb = load_neighbour(row, kb + lane, kmax, true, s_xyz, ns, qx, qy, qz, DX ? nullptr : flag);
    const int nv = stage_neighbours<INFL, AGG>(nb, a, infl, ids, lane, cnt);
    for (int c0 = 0; c0 < nchunk; ++c0) {
      const int c = c0 * 64 + lane;
      const bool cok = c < cin;
      float acc[kKPmax];
#pragma unroll
      for (int p = 0; p < kKPmax; ++p) acc[p] = 0.f;
      if constexpr (!DX) {
        walk_neighbours<INFL, AGG, false>(x + (cok ? c : 0), cok, cin, nv, infl, ids, 0, acc);
        // (kmax <= 64: one pass, plain store; wider rows: later passes add to what the first wrote)
        if (cok) {
#pragma unroll
          for (int p = 0; p < kKPmax; ++p)
            if (p < a.n_kp) {
              float* dst = wf + ((size_t)n * a.n_kp + p) * cin + c;
              const float v = ONE_SUM ? acc[0] : acc[p];
              *dst = kb == 0 ? v : *dst + v;
            }
        }
      } else {
        float gsum = 0.f;   // constant / sum: every influence is 1
#pragma unroll
        for (int p = 0; p < kKPmax; ++p) {
          acc[p] = (cok && p < a.n_kp) ? dwf[((size_t)n * a.n_kp + p) * cin + c] : 0.f;
          gsum += acc[p];
        }
        for (int k = 0; k < nv; ++k) {
          const float* iw = infl + k * slot_floats(AGG);
          float v;
          if constexpr (AGG == SPR_KP_CLOSEST) {
            const float2 wp = *reinterpret_cast<const float2*>(iw);
            float g = 0.f;
            switch (__builtin_amdgcn_readfirstlane(__float_as_int(wp.y))) {
#define SPR_KP_SEL(P) \
  case P:             \
    g = acc[P];       \
    break;
              SPR_KP_CASES(SPR_KP_SEL)
#undef SPR_KP_SEL
            }
            v = wp.x * g;
          } else if constexpr (ONE_SUM) {
            v = gsum;
          } else {
            v = 0.f;
#pragma unroll
            for (int p4 = 0; p4 < kKPmax / 4; ++p4) {
              const float4 w4 = *reinterpret_cast<const float4*>(iw + 4 * p4);
              v += w4.x * acc[4 * p4];
              v += w4.y * acc[4 * p4 + 1];
              v += w4.z * acc[4 * p4 + 2];
              v += w4.w * acc[4 * p4 + 3];
            }
          }
          if (cok && v != 0.f) fx_add(dx_acc + (size_t)ids[k] * cin + c, v, fx);
        }
      }
    }
  }
  if (!DX && lane == 0) cnt_out[n] = (float)max(cnt, 1);
}

#undef SPR_KP_CASES

// the workspace of the forward: the flags of launch_rowflag, then what spr_kpconv_fwd keeps for its tile kernel
struct ModesWs {
  unsigned char* flag;
  float4* sxf;             // launch_rowflag's support records (unused here; it writes them)
  int* tile_ctr;
  unsigned char* wplanes;  // spr_kpconv_wplanes_bytes(cin, cout) when the shape has planes
  float *x_parts, *w_parts;
};
inline bool modes_plane_shape(int cin, int cout) { return cin > 0 && cin % 32 == 0 && cout > 0 && cout % 32 == 0 && cout <= 256; }
ModesWs modes_layout(Workspace& w, int nq, int ns, int cin, int cout) {
  (void)nq;
  const size_t n = (size_t)(ns > 0 ? ns : 1);
  ModesWs l;
  l.flag = w.take<unsigned char>(n);
  l.sxf = w.take<float4>(n + 1);
  l.tile_ctr = w.take<int>(64);
  l.wplanes = w.take<unsigned char>(modes_plane_shape(cin, cout) ? spr_kpconv_wplanes_bytes(cin, cout) : 0);
  l.x_parts = w.take<float>(kAmaxParts);
  l.w_parts = w.take<float>(kAmaxParts);
  return l;
}
struct ModesFlagWs {
  unsigned char* flag;
  float4* sxf;
  int* tile_ctr;
};
ModesFlagWs modes_flag_layout(Workspace& w, int ns) {
  const size_t n = (size_t)(ns > 0 ? ns : 1);
  ModesFlagWs l;
  l.flag = w.take<unsigned char>(n);
  l.sxf = w.take<float4>(n + 1);
  l.tile_ctr = w.take<int>(64);
  return l;
}

int check_mode(const char* what, int influence, int aggregation) {
  SPR_REQUIRE(influence == SPR_KP_CONSTANT || influence == SPR_KP_LINEAR || influence == SPR_KP_GAUSSIAN,
              "%s: unknown influence %d", what, influence);
  SPR_REQUIRE(aggregation == SPR_KP_SUM || aggregation == SPR_KP_CLOSEST, "%s: unknown aggregation %d", what,
              aggregation);
  return 0;
}
KpModeArgs mode_args(const float* kernel_points, int n_kp, float kp_extent) {
  const double sigma = (double)kp_extent * 0.3;   // the reference forms 2 sigma^2 + eps as a Python float
  return KpModeArgs{kernel_points, n_kp, 1.0f / kp_extent, (float)(2.0 * sigma * sigma + 1e-9)};
}

// F<INFL, AGG>::run(args...) for the runtime (influence, aggregation); both were checked by check_mode
template <template <int, int> class F, typename... Args>
int dispatch_mode(int influence, int aggregation, Args... args) {
#define SPR_KP_MODE(I, A) \
  if (influence == I && aggregation == A) return F<I, A>::run(args...);
  SPR_KP_MODE(SPR_KP_CONSTANT, SPR_KP_SUM)
  SPR_KP_MODE(SPR_KP_LINEAR, SPR_KP_SUM)
  SPR_KP_MODE(SPR_KP_GAUSSIAN, SPR_KP_SUM)
  SPR_KP_MODE(SPR_KP_CONSTANT, SPR_KP_CLOSEST)
  SPR_KP_MODE(SPR_KP_LINEAR, SPR_KP_CLOSEST)
  SPR_KP_MODE(SPR_KP_GAUSSIAN, SPR_KP_CLOSEST)
#undef SPR_KP_MODE
  return 2;
}

template <int INFL, int AGG>
struct TileLaunch {
  template <typename... Args>
  static int run(int cc, Args... args) {
    return cc == 64 ? launch_modes_tile<INFL, AGG, 64>(args...) : launch_modes_tile<INFL, AGG, 32>(args...);
  }
};
template <int INFL, int AGG>
struct WfLaunch {
  static int run(const float* q_xyz, int nq, const float* s_xyz, int ns, const int* nbr, int nbr_stride, int kmax,
                 const float* x, int cin, KpModeArgs a, float* wf, float* cnt, const unsigned char* flag,
                 hipStream_t stream) {
    hipLaunchKernelGGL((k_kpconv_modes_aux<INFL, AGG, false>), dim3(cdiv(nq, 4)), dim3(256), 0, stream, q_xyz, nq, s_xyz,
                       ns, nbr, nbr_stride, kmax, x, cin, a, (const float*)nullptr, wf, cnt, flag,
                       (const float*)nullptr, (unsigned long long*)nullptr);
    return 0;
  }
};
template <int INFL, int AGG>
struct DxLaunch {
  static int run(const float* q_xyz, int nq, const float* s_xyz, int ns, const int* nbr, int nbr_stride, int kmax,
                 int cin, KpModeArgs a, const float* dwf, const float* parts, unsigned long long* acc,
                 hipStream_t stream) {
    hipLaunchKernelGGL((k_kpconv_modes_aux<INFL, AGG, true>), dim3(cdiv(nq, 4)), dim3(256), 0, stream, q_xyz, nq, s_xyz,
                       ns, nbr, nbr_stride, kmax, (const float*)nullptr, cin, a, dwf, (float*)nullptr, (float*)nullptr,
                       (const unsigned char*)nullptr, parts, acc);
    return 0;
  }
};

}  // namespace
}  // namespace spr

using namespace spr;

extern "C" size_t spr_kpconv_modes_workspace_size(int nq, int ns, int cin, int cout) {
  return measure(modes_layout, nq, ns, cin, cout);
}

extern "C" int spr_kpconv_modes_fwd(const float* q_xyz, int nq, const float* s_xyz, int ns, const int* nbr,
                                    int nbr_stride, int kmax, const float* x, int cin, const float* weights, int cout,
                                    const float* kernel_points, int n_kp, float kp_extent, int influence,
                                    int aggregation, float* out, int impl, const float* x_range, int x_range_n,
                                    const float* w_range, int w_range_n, const void* wplanes, void* ws,
                                    size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (int rc = check_mode("kpconv_modes", influence, aggregation)) return rc;
  SPR_REQUIRE((x_range == nullptr || x_range_n >= 1) && (w_range == nullptr || w_range_n >= 1),
              "kpconv_modes: a range needs a count");
  SPR_REQUIRE(nq > 0 && ns > 0, "kpconv_modes: empty input");
  SPR_REQUIRE(kmax >= 1 && kmax <= nbr_stride, "kpconv_modes: bad kmax=%d stride=%d", kmax, nbr_stride);
  SPR_REQUIRE(cin >= 1 && cout >= 1 && n_kp >= 1 && n_kp <= 32, "kpconv_modes: bad dims");
  SPR_REQUIRE(kp_extent > 0.f, "kpconv_modes: KP_extent must be > 0");
  SPR_REQUIRE(impl == 0 || impl == 1, "kpconv_modes: impl is 0 or 1");
  Workspace w(ws, ws_bytes);
  const ModesWs l = modes_layout(w, nq, ns, cin, cout);
  SPR_REQUIRE(ws != nullptr && w.ok(), "kpconv_modes: workspace too small");
  SPR_REQUIRE(wplanes == nullptr || w_range != nullptr,
              "kpconv_modes: prepared weight planes come with the range they were scaled by");
  const KpModeArgs a = mode_args(kernel_points, n_kp, kp_extent);

  launch_rowflag(x, s_xyz, ns, cin, l.flag, l.sxf, l.tile_ctr, stream);
  SPR_LAUNCH_CHECK();

  if (impl == 0 && n_kp == kKP && modes_plane_shape(cin, cout)) {
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
    return dispatch_mode<TileLaunch>(influence, aggregation, cin % 64 == 0 ? 64 : 32, q_xyz, nq, s_xyz, ns, nbr,
                                     nbr_stride, kmax, x, cin, wh, wl, cout, a, (const unsigned char*)l.flag, xp, wp,
                                     n_xp, n_wp, out, stream);
  }
  const long total = (long)nq * cout;
  hipLaunchKernelGGL(k_kpconv_modes_simple, dim3(cdiv(total, 256)), dim3(256), 0, stream, q_xyz, nq, s_xyz, ns, nbr,
                     nbr_stride, kmax, x, cin, weights, cout, a, influence, aggregation, l.flag, out);
  SPR_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t spr_kpconv_modes_weighted_features_workspace_size(int ns) {
  return measure(modes_flag_layout, ns);
}

extern "C" int spr_kpconv_modes_weighted_features(const float* q_xyz, int nq, const float* s_xyz, int ns,
                                                  const int* nbr, int nbr_stride, int kmax, const float* x, int cin,
                                                  const float* kernel_points, int n_kp, float kp_extent,
                                                  int influence, int aggregation, float* wf, float* cnt, void* ws,
                                                  size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (int rc = check_mode("kpconv_modes_weighted_features", influence, aggregation)) return rc;
  SPR_REQUIRE(nq > 0 && ns > 0 && cin >= 1 && n_kp >= 1 && n_kp <= kKPmax && kp_extent > 0.f && kmax >= 1 &&
                  kmax <= nbr_stride, "kpconv_modes_weighted_features: bad arguments");
  Workspace w(ws, ws_bytes);
  const ModesFlagWs l = modes_flag_layout(w, ns);
  SPR_REQUIRE(ws != nullptr && w.ok(), "kpconv_modes_weighted_features: workspace too small");
  launch_rowflag(x, s_xyz, ns, cin, l.flag, l.sxf, l.tile_ctr, stream);
  if (int rc = dispatch_mode<WfLaunch>(influence, aggregation, q_xyz, nq, s_xyz, ns, nbr, nbr_stride, kmax, x, cin,
                                       mode_args(kernel_points, n_kp, kp_extent), wf, cnt,
                                       (const unsigned char*)l.flag, stream))
    return rc;
  SPR_LAUNCH_CHECK();
  return 0;
}

extern "C" int spr_kpconv_modes_bwd_dx(const float* q_xyz, int nq, const float* s_xyz, int ns, const int* nbr,
                                       int nbr_stride, int kmax, int cin, const float* kernel_points, int n_kp,
                                       float kp_extent, int influence, int aggregation, const float* dwf,
                                       const float* dwf_range, int dwf_range_n, float* dx, void* ws, size_t ws_bytes,
                                       void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (int rc = check_mode("kpconv_modes_bwd_dx", influence, aggregation)) return rc;
  SPR_REQUIRE(dwf_range == nullptr || dwf_range_n >= 1, "kpconv_modes_bwd_dx: a range needs a count");
  SPR_REQUIRE(nq > 0 && ns > 0 && cin >= 1 && n_kp >= 1 && n_kp <= kKPmax && kp_extent > 0.f && kmax >= 1 &&
                  kmax <= nbr_stride, "kpconv_modes_bwd_dx: bad arguments");
  FxScratch f;
  if (int rc = fx_scratch(ws, ws_bytes, ns, cin, stream, &f)) return rc;
  if (dwf_range != nullptr) {
    hipLaunchKernelGGL(k_range_to_parts, dim3(1), dim3(256), 0, stream, dwf_range, dwf_range_n, f.parts);
  } else if (int rc = launch_absmax(dwf, nq, n_kp * cin, n_kp * cin, f.parts, stream)) {
    return rc;
  }
  if (int rc = dispatch_mode<DxLaunch>(influence, aggregation, q_xyz, nq, s_xyz, ns, nbr, nbr_stride, kmax, cin,
                                       mode_args(kernel_points, n_kp, kp_extent), dwf, (const float*)f.parts, f.acc,
                                       stream))
    return rc;
  hipLaunchKernelGGL(k_fx_to_float, dim3(cdiv((long)ns * cin, 256)), dim3(256), 0, stream, f.acc, (long)ns * cin,
                     f.parts, (float)n_kp, dx);
  SPR_LAUNCH_CHECK();
  return 0;
}
