// Buffer descriptors, LDS-DMA pieces and counted vmcnt waits: the one definition shared by the kernels that issue
// `buffer_load_dwordx4 ... offen lds` in inline asm (conv_bt, conv64_dma, conv_pw, the weight-gradient rings) and by the
// branch-free raw-buffer kernels (conv64, conv_mma_fast, wgrad_tile).
#pragma once
#include "common.h"

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef __amdgpu_buffer_rsrc_t rsrc_t;
constexpr unsigned SENT = 0xFFFFFFF0u;  // always beyond num_records: loads return zero, stores are dropped

// descriptor for the raw_buffer builtins
__device__ __forceinline__ rsrc_t make_rsrc(const void* p, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, (int)bytes, 0x00020000);
}
// the same descriptor as four wave-uniform words, for the "s" operand of an asm statement
__device__ __forceinline__ i32x4 rsrc_words(const void* p, unsigned bytes) {
  const unsigned long long addr = (unsigned long long)p;
  i32x4 r;
  r.x = __builtin_amdgcn_readfirstlane((int)(unsigned)addr);
  r.y = __builtin_amdgcn_readfirstlane((int)(unsigned)(addr >> 32));
  r.z = __builtin_amdgcn_readfirstlane((int)bytes);
  r.w = 0x00020000;
  return r;
}

// One LDS-DMA piece: 64 lanes x 16 bytes, lane L lands at lds_dst + 16 L.  M0 (the LDS base) is written and read inside this
// one statement (hipcc uses M0 for nothing else in these kernels); s_nop NOP covers the VALU-written-SGPR -> VMEM hazard of the
// descriptor / offset operands, which hipcc does not pad inside an asm statement: NOP = 4 in conv_bt, conv64_dma and conv_pw.
// The weight-gradient kernels have always used 0 (weight-gradient section, open question).
// Two overloads: with a wave-uniform `soff` SGPR, and with the literal 0 in its place (a zero passed through "s" costs a register).
template <int NOP>
__device__ __forceinline__ void dma16(i32x4 rsrc, unsigned voff, unsigned soff, unsigned lds_dst) {
  asm volatile("s_mov_b32 m0, %3\n\ts_nop %4\n\tbuffer_load_dwordx4 %0, %1, %2 offen lds" : : "v"(voff), "s"(rsrc), "s"(soff), "s"(lds_dst), "n"(NOP) : "memory", "m0");
}
template <int NOP>
__device__ __forceinline__ void dma16(i32x4 rsrc, unsigned voff, unsigned lds_dst) {
  asm volatile("s_mov_b32 m0, %2\n\ts_nop %3\n\tbuffer_load_dwordx4 %0, %1, 0 offen lds" : : "v"(voff), "s"(rsrc), "s"(lds_dst), "n"(NOP) : "memory", "m0");
}

// wait until at most N vector-memory operations of this wave are outstanding
template <int N> __device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
