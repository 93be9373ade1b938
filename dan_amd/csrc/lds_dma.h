// The LDS-DMA layer of the streaming kernels (conv_halo*.hip, conv_pointwise.hip, conv_wgrad_rows.hip, conv_wgrad_pw.hip, deform_fused.hip):
// the raw buffer descriptor, the 16-byte-per-lane DMA, the counted wait that retires it and the two 32-byte-slot LDS swizzles.  One
// definition: a change to the descriptor flags, to the M0 handling or to a swizzle bit reaches every kernel that streams through it.
#pragma once
#include "common.h"

typedef __attribute__((ext_vector_type(4))) unsigned dh_u32x4;

// At most N vector-memory operations of this wave stay outstanding (N a compile-time constant: the kernels count their DMAs by hand).
template <int N>
__device__ __forceinline__ void dh_wait_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// 16-byte-per-lane LDS-DMA as inline asm: hipcc counts a builtin LDS-DMA as a pending LDS write and drains it (vmcnt(0)) in front of
// the next ds_read it cannot prove disjoint — every K-step of a streaming loop.  Hidden in asm the DMA is counted by hand (dh_wait_vmcnt)
// and stays in flight across the barriers.  A lane whose voff is out of the descriptor's range (0xFFFFFFFF) writes ZEROS to its LDS slot.
// M0 (the LDS destination base) is written in the statement that uses it and restored after.
__device__ __forceinline__ void dh_dma16(dh_u32x4 rsrc, unsigned voff, unsigned lds_addr) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(voff), "s"(rsrc), "s"(lds_addr) : "memory");
}
__device__ __forceinline__ dh_u32x4 dh_make_rsrc(const void* p, unsigned bytes) {   // raw buffer descriptor: base, stride 0, num_records, flags
  const unsigned long long a = (unsigned long long)p;
  return dh_u32x4{(unsigned)a, (unsigned)(a >> 32) & 0xFFFFu, bytes, 0x00020000u};
}

// 32-byte-slot swizzles of a [pixel][channel] LDS tile: the key (in 32-byte slots) XORed into a pixel's 16-byte chunk index, for 128-byte
// and 256-byte pixel rows
__device__ __forceinline__ int dh_swz128(int pc) { return ((pc >> 1) & 1) | (((pc >> 3) & 1) << 1); }
__device__ __forceinline__ int dh_swz256(int px) { return (px & 3) | (((px >> 3) & 1) << 2); }
