// LDS-DMA (global_load_lds_*) and counted vector-memory waits: the only place these asm statements exist.
// Users: k_kpconv_ring (kpconv.hip), k_xenc_chain (xenc.hip), k_attn_s (attention.hip); linear.hip and the KPConv tile
// kernel use the waits alone.
//
// The instruction.  global_load_lds_dword / _dwordx4 moves 4 / 16 bytes per active lane from
//   base (SGPR pair) + off (per-lane VGPR byte offset) + the immediate offset
// to LDS at
//   M0 + the immediate offset + 4 / 16 * lane
// without passing through vector registers.  The immediate offset moves BOTH addresses, so further pieces of one block
// are the same instruction with another immediate.  The compiler does not see the LDS write and does not count the
// load: the caller orders it against its own LDS reads (lgkmcnt) and retires it with the counted waits below.
//
// Contract.
//   M0 rule.  An LDS-DMA needs one wait state behind a write of M0.  Every statement here that writes M0 holds the
//     write, the wait state (s_nop 0) and the first use together, so nothing can come between them.
//   Two M0 conventions; each function says which it follows.
//     "sets M0": leaves M0 changed and names "m0" as clobbered, so the compiler keeps nothing in it across the
//       statement.  The pieces with an immediate offset (lds_dma16_more) write no M0: they use what the
//       lds_dma16_first in front of them left there, and name "m0" so that the compiler treats the group alike.
//     "keeps M0": saves and restores M0 inside the statement and names no clobber.
//   Base operand.  `base` is an "s" operand: the instruction reads it from an SGPR pair, so it must be wave uniform
//     (a kernel argument, or built from readfirstlane results).  A uniform value the compiler has SPILLED is no longer
//     one: it comes back by lane reads (v_readlane) placed by the compiler next to the statement, and a spilled SGPR
//     beside an "s"(pointer) operand has cost a GPU memory fault here.  So these functions are safe only in a kernel
//     the build proves free of scratch and SGPR spills: csrc/Makefile runs usage_check.py over every instantiation of
//     the three kernels named above.  The same holds for M0 between the pieces of a group: SGPR spill code writes it.
//   Counted waits.  s_waitcnt vmcnt(N) returns once at most N vector-memory operations of the wave are outstanding.
//     A count may assume that loads return in issue order (the N youngest may be in flight, everything older has
//     landed; stores count too, in order with the loads), and must remember that loads and stores the COMPILER issued
//     share the counter: a count is valid only where the caller knows every vector-memory instruction between the
//     DMA and the wait.  An under-count only waits longer; an over-count reads LDS that has not arrived.
#pragma once
#include <hip/hip_runtime.h>

namespace spr {

// at most N vector-memory operations of this wave outstanding
template <int N>
__device__ __forceinline__ void wait_vm() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
// A wait whose count is a run-time (wave-uniform) value, or one that folds to a constant only after unrolling: a switch
// over an EXPLICIT list of the counts the caller can ask for; any other value waits for everything.
//   #define MY_COUNTS(W) W(0) W(4) W(8)
//   SPR_DEFINE_WAIT_VM_ANY(wait_vm_mine, MY_COUNTS)          ->  void wait_vm_mine(int n)
// (A list generated from an integer_sequence compiles to other compare / branch polarities in k_kpconv_ring.)
#define SPR_WAIT_VM_CASE(k) case k: wait_vm<k>(); break;
#define SPR_DEFINE_WAIT_VM_ANY(name, COUNTS)           \
  __device__ __forceinline__ void name(int n) {        \
    switch (n) {                                       \
      COUNTS(SPR_WAIT_VM_CASE)                         \
      default: wait_vm<0>(); break;                    \
    }                                                  \
  }

// 16 bytes per active lane from base + off to LDS at dst_s + 16 * lane.  Sets M0.
__device__ __forceinline__ void lds_dma16_first(const void* base, unsigned off, unsigned dst_s) {
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1"
               : : "v"(off), "s"(base), "s"(dst_s) : "memory", "m0");
}
// Piece Q (1 KiB = one wave instruction each) behind an lds_dma16_first: base + off + Q KiB to M0 + Q KiB + 16 * lane.
// The bare instruction: relies on nothing having written M0 since that lds_dma16_first ("sets M0" convention).
template <int Q>
__device__ __forceinline__ void lds_dma16_more(const void* base, unsigned off) {
  asm volatile("global_load_lds_dwordx4 %0, %1 offset:%2" : : "v"(off), "s"(base), "n"(Q * 1024) : "memory", "m0");
}
// One KPConv ring item behind ONE M0 setup: PPI (1 or 2) 1-KiB pieces of feature rows to dst_s (+ 1 KiB), then 8
// records of 16 bytes (lanes 0..7 only; exec is restored inside the statement) to dst_s + 8 * RB.  The second piece and
// the records are issued against bases the caller has moved DOWN by their LDS displacement (x_m1k = x - 1024,
// sx_m = records - 8 * RB), since the immediate offset moves both addresses.  Sets M0.
template <int PPI, int RB>
__device__ __forceinline__ void lds_dma_ring_item(const void* x, const void* x_m1k, const void* sx_m, unsigned off0,
                                                  unsigned off1, unsigned off_rec, unsigned dst_s) {
  static_assert(PPI == 1 || PPI == 2, "ring item: one or two row pieces");
  unsigned long long keep;
  if constexpr (PPI == 2) {
    asm volatile(
        "s_mov_b32 m0, %7\n\ts_nop 0\n\t"
        "global_load_lds_dwordx4 %1, %4\n\t"
        "global_load_lds_dwordx4 %2, %5 offset:1024\n\t"
        "s_mov_b64 %0, exec\n\ts_mov_b64 exec, 0xff\n\t"
        "global_load_lds_dwordx4 %3, %6 offset:%8\n\t"
        "s_mov_b64 exec, %0"
        : "=&s"(keep) : "v"(off0), "v"(off1), "v"(off_rec), "s"(x), "s"(x_m1k), "s"(sx_m), "s"(dst_s), "n"(8 * RB)
        : "memory", "m0");
  } else {
    asm volatile(
        "s_mov_b32 m0, %5\n\ts_nop 0\n\t"
        "global_load_lds_dwordx4 %1, %3\n\t"
        "s_mov_b64 %0, exec\n\ts_mov_b64 exec, 0xff\n\t"
        "global_load_lds_dwordx4 %2, %4 offset:%6\n\t"
        "s_mov_b64 exec, %0"
        : "=&s"(keep) : "v"(off0), "v"(off_rec), "s"(x), "s"(sx_m), "s"(dst_s), "n"(8 * RB)
        : "memory", "m0");
  }
}
// 4 bytes per active lane from base + off to LDS at dst_s + 4 * lane.  Keeps M0.  The lgkmcnt(0) in front orders the
// write behind every ds_read this wave has issued (the words being overwritten).
__device__ __forceinline__ void lds_dma4(const void* base, unsigned off, unsigned dst_s) {
  unsigned keep;
  asm volatile(
      "s_waitcnt lgkmcnt(0)\n\ts_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"
      "global_load_lds_dword %1, %2\n\ts_mov_b32 m0, %0"
      : "=&s"(keep) : "v"(off), "s"(base), "s"(dst_s) : "memory");
}

}  // namespace spr
