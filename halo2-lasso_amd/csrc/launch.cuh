// What the kernel files share around a launch: the grid-stride loop, the two grid rules, the run-time value -> template
// argument dispatch and the host-side weight scaling of the wide accumulator (wide.cuh).  Included by the kernels_*.hip files only; none of it is device code of its own.
#pragma once
#include <hip/hip_runtime.h>
#include <string.h>
#include <algorithm>
#include <type_traits>
#include "dev.hpp"
#include "ff.cuh"
#include "ff_host.hpp"

namespace lh {

#define GSTRIDE(i, n) \
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (size_t)gridDim.x * blockDim.x)

// ceil(n / block) workgroups, at least one and at most `cap`
static inline dim3 grid_for(size_t n, int block = 256, size_t cap = 4096) {
  size_t g = (n + block - 1) / block;
  if (g < 1) g = 1;
  if (g > cap) g = cap;
  return dim3((unsigned)g);
}
// the CU-bounded grid of the streaming kernels: ceil(work / per_block) workgroups, at least one and at most 8 per CU
static inline unsigned cu_grid(const Ctx& c, size_t work, size_t per_block = 256) {
  return (unsigned)std::max<size_t>(1, std::min<size_t>((work + per_block - 1) / per_block, (size_t)c.num_cus * 8));
}

// f(std::integral_constant<int, V>) for the V in [LO, HI] that equals v (a v beyond HI takes HI: callers check the range):
//   dispatch_int<1, 6>(degree, [&](auto D) { hipLaunchKernelGGL((kernel<D()>), ...); });
template <int LO, int HI, class F>
static inline void dispatch_int(int v, F&& f) {
  if constexpr (LO == HI) {
    f(std::integral_constant<int, LO>{});
  } else {
    if (v == LO) f(std::integral_constant<int, LO>{});
    else dispatch_int<LO + 1, HI>(v, f);
  }
}
template <class F>
static inline void dispatch_bool(bool v, F&& f) {
  if (v) f(std::true_type{});
  else f(std::false_type{});
}

// host: w (Montgomery form) -> w R (Montgomery form), the weight wide_redc expects
static inline Fr prescale_r(const Fr& w) {
  static const host::Fr scale = [] {
    uint64_t c[4];
    for (int k = 0; k < 4; k++) c[k] = (uint64_t)FrParams::r1(2 * k) | ((uint64_t)FrParams::r1(2 * k + 1) << 32);
    return host::Fr::from_canonical(c);  // the field element R mod r
  }();
  host::Fr h;
  memcpy(&h, &w, sizeof(h));
  h = h * scale;
  Fr out;
  memcpy(&out, &h, sizeof(out));
  return out;
}

}  // namespace lh
