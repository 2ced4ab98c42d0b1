// Wide integer accumulation of Fr weights times small integers (device only): the small-valued column kernels of
// kernels_poly.hip, kernels_logup.hip, kernels_memcheck.hip, kernels_spark.hip and kernels_brakedown.hip and the field-edge
// probe (ff_probe.hip) include it.
#pragma once
#include "ff.cuh"

namespace lh {

// ------------------------------------------------------------------ small-valued columns (Lasso's dim / read_ts / E / final_cts)
// A Montgomery residue W = w R mod r times a 32-bit integer v is 8 multiply-adds into a 10-limb integer accumulator
// (no reduction); a sum T of such products is reduced ONCE:  T mod r = mont(T_lo, R mod r) + (T_hi R mod r)  - the
// Montgomery product with the residue of one reduces any 256-bit integer, the high limbs re-enter as Fr::from(T_hi).
// A term costs 8 v_mad_u64_u32 instead of the 129 + 129 of from_u64 followed by mul.
struct Wide {
  uint32_t l[10];
  __device__ __forceinline__ static Wide zero() {
    Wide w;
#pragma unroll
    for (int k = 0; k < 10; k++) w.l[k] = 0;
    return w;
  }
};
__device__ __forceinline__ void wide_mac(Wide& acc, const Fr& w, uint32_t v) {
  uint64_t carry = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const uint64_t t = (uint64_t)w.l[k] * v + acc.l[k] + carry;  // < 2^64: (2^32-1)^2 + 2 (2^32-1)
    acc.l[k] = (uint32_t)t;
    carry = t >> 32;
  }
  const uint64_t t = (uint64_t)acc.l[8] + carry;
  acc.l[8] = (uint32_t)t;
  acc.l[9] += (uint32_t)(t >> 32);
}
__device__ __forceinline__ Fr wide_reduce(const Wide& acc) {
  Fr lo;
#pragma unroll
  for (int k = 0; k < 8; k++) lo.l[k] = acc.l[k];
  const Fr one = from_u64<FrParams>(1);  // R mod r
  const uint64_t hi = (uint64_t)acc.l[8] | ((uint64_t)acc.l[9] << 32);
  Fr r = mul(lo, one);  // lo < 2^256, one < r: the product-scanning multiplication stays below 2 r (ff.cuh)
  if (hi) r = add(r, from_u64<FrParams>(hi));
  return r;
}

// The same sum with weights given TIMES R (w R^2 in memory, prescale_r on the host): one Montgomery REDUCTION of the
// 10-limb accumulator (72 multiply-adds) returns sum_k w_k v_k in Montgomery form, instead of the two full
// multiplications of wide_reduce (258).  acc < 2^320, so the result is below 2^64 + r < 2 r: one conditional subtraction.
__device__ __forceinline__ Fr wide_redc(const Wide& acc) {
  uint32_t a[18];
#pragma unroll
  for (int k = 0; k < 10; k++) a[k] = acc.l[k];
#pragma unroll
  for (int k = 10; k < 18; k++) a[k] = 0u;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint32_t m = a[i] * FrParams::INV;
    uint64_t carry = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const uint64_t t = (uint64_t)m * FrParams::mod(j) + a[i + j] + carry;
      a[i + j] = (uint32_t)t;
      carry = t >> 32;
    }
#pragma unroll
    for (int j = i + 8; j < 18; j++) {
      const uint64_t t = (uint64_t)a[j] + carry;
      a[j] = (uint32_t)t;
      carry = t >> 32;
    }
  }
  Fr r;
#pragma unroll
  for (int k = 0; k < 8; k++) r.l[k] = a[8 + k];
  return reduce_once(r);
}
// a 32-bit integer as a field element: 8 multiply-adds and one reduction (one_r = R^2 mod r, the prescaled one)
__device__ __forceinline__ Fr wide_small(const Fr& one_r, uint32_t v) {
  Wide w = Wide::zero();
  wide_mac(w, one_r, v);
  return wide_redc(w);
}

}  // namespace lh
