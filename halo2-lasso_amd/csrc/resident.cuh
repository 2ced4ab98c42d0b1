// Device-side pieces shared by the resident kernels (kernels_sumcheck.hip sc_tail_kernel, kernels_gkr.hip): 16-byte
// system-scope accesses and the self-validating message chunks (dev.hpp TailChunk).  The ticket between their workgroups is
// round.cuh draw_ticket, by wave 0's thread 0 once the wave's stores have left.
#pragma once
#include <hip/hip_runtime.h>
#include "dev.hpp"
#include "round.cuh"

namespace lh {

__device__ __forceinline__ Fr shfl_xor_fr(const Fr& v, int mask) {
  Fr o;
#pragma unroll
  for (int i = 0; i < 8; i++) o.l[i] = __shfl_xor(v.l[i], mask, 64);
  return o;
}

// 16-byte system-scope accesses: one request to host memory each
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ u32x4 load_sys_x4(const void* p) {
  u32x4 v;
  asm volatile("global_load_dwordx4 %0, %1, off sc0 sc1\n\ts_waitcnt vmcnt(0)" : "=v"(v) : "v"(p) : "memory");
  return v;
}
__device__ __forceinline__ void store_sys_x4(void* p, u32x4 v) {
  asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1" ::"v"(p), "v"(v) : "memory");
}
__device__ __forceinline__ void tail_send(TailChunk* msg, uint32_t x, const Fr& s, uint32_t seq) {
  store_sys_x4(&msg[3 * x + 0], u32x4{seq, s.l[0], s.l[1], s.l[2]});
  store_sys_x4(&msg[3 * x + 1], u32x4{seq, s.l[3], s.l[4], s.l[5]});
  store_sys_x4(&msg[3 * x + 2], u32x4{seq, s.l[6], s.l[7], 0u});
}

}  // namespace lh
