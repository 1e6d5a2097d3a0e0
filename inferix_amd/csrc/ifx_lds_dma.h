// LDS-DMA (global memory -> LDS without staging registers) as every kernel of the library issues it, ONCE: the address-space pointer
// types of the builtin form, the buffer-descriptor form and its descriptor, and the waits that go with either.  Device only.
// Users: ifx_gemm_glds.hip, ifx_quant.hip (builtin form, through ifx_gemm_tile.h); ifx_gemm_pp.hip, ifx_conv.hip, ifx_attn_pp.hip
// (descriptor form).
#pragma once
#include <hip/hip_runtime.h>

namespace ifx {

// what __builtin_amdgcn_global_load_lds takes; (unsigned)(unsigned long long)(lds_ptr_t)smem is the LDS byte address of `smem`
typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef const __attribute__((address_space(1))) void* gbl_ptr_t;
typedef int v4i __attribute__((ext_vector_type(4)));

// One LDS-DMA instruction (64 lanes x 16 B, lane-linear at LDS byte address `lds`), issued from inline asm ON PURPOSE:
// hipcc tracks the LDS-DMA builtins as LDS stores and puts `s_waitcnt vmcnt(0)` in front of the next ds_read that
// might alias them — in a ping-pong loop every fragment read of the MFMA step — which drains the whole prefetch queue once per tile.
// The ring discipline of the caller (counted vmcnt + workgroup barrier before a slot is read) is what orders DMA and reads.
__device__ __forceinline__ void dma16(v4i rsrc, unsigned lds, int voff, int soff) {
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds"
               :
               : "s"(lds), "v"(voff), "s"(rsrc), "s"(soff)
               : "memory");      // m0 is a reserved register: hipcc sets it itself right before each of its own uses
}
__device__ __forceinline__ void dma4(v4i rsrc, unsigned lds, int voff) {      // 4 bytes per lane (a cache-line touch: the data is not used)
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dword %1, %2, 0 offen lds" : : "s"(lds), "v"(voff), "s"(rsrc) : "memory");
}
__device__ __forceinline__ v4i make_rsrc(const void* base, unsigned num_bytes) {
  const unsigned long long a = (unsigned long long)base;
  v4i r;
  r[0] = (int)(unsigned)a;
  r[1] = (int)((unsigned)(a >> 32) & 0xffffu);      // stride 0: raw buffer, byte offsets, reads past num_bytes return 0
  r[2] = (int)num_bytes;
  r[3] = 0x00020000;
  return r;
}

// at most N vector-memory instructions (LDS-DMA pieces included) of this wave still in flight
template <int N>
__device__ __forceinline__ void wait_vm() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
// lgkmcnt(0) through the builtin (simm16: vmcnt 63, expcnt 7, lgkmcnt 0), so that hipcc's own scoreboard knows the fragment reads have
// returned: after an asm wait it keeps protecting their registers with lgkmcnt(14 .. 0) in the middle of the next batch of reads
__device__ __forceinline__ void wait_lds() { __builtin_amdgcn_s_waitcnt(0xC07F); }

}  // namespace ifx
