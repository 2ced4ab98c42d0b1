// The wave steps of the keyed field sums (kernels_spartan.hip spartan_spmv, kernels_nova.hip nova_spmv2): the segmented scan of
// one wave row of a key-sorted stream and what a scanned wave stores or carries.  Device only.
#pragma once
#include <hip/hip_runtime.h>
#include "dev.hpp"
#include "ff.cuh"

namespace lh {

// A workgroup of 256 lanes takes one tile of SPMV_TILE consecutive sorted entries as SPMV_TILE / 64 wave rows of 64 entries;
// the open head and tail of every wave row are 2 * SPMV_TILE / 64 = 64 carry items: one wave's worth, by design.
static_assert(SPMV_TILE == 2048 && SPMV_TILE <= 4096, "the tile's carry items are folded by ONE wave");
constexpr int SPMV_ROWS = SPMV_TILE / 64;
constexpr uint32_t SPMV_NO_KEY = 0xFFFFFFFFu;  // (keys are masked to dim_vars <= 24 bits: no entry has it)

// One wave, lane t holding (key, v) of item t of a stream with EQUAL KEYS ADJACENT: the inclusive sum of v over the items of
// t's segment up to t (Hillis-Steele over wave shuffles: with adjacent equal keys, key[t - off] == key[t] says that every
// item between belongs to the segment too).  tail: t is the last item of its segment inside the wave; from0: its segment
// holds item 0.
__device__ __forceinline__ Fr wave_segmented_sum(uint32_t key, Fr v, bool& tail, bool& from0) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t ko = __shfl_up(key, off, 64);
    Fr o;
#pragma unroll
    for (int i = 0; i < 8; i++) o.l[i] = __shfl_up(v.l[i], off, 64);
    if (lane >= off && ko == key) v = add(v, o);
  }
  tail = lane == 63 || __shfl_down(key, 1, 64) != key;
  from0 = __shfl(key, 0, 64) == key;
  return v;
}

// What a scanned wave does with its sums: a segment closed inside the wave (neither item 0 nor item 63 in it) is stored
// straight - nobody else holds a part of it, the stream being sorted -; the segment of item 0 and the one of item 63 may go
// on outside and leave as the two carry items (head, tail) at ck / cv [0], [1].  One segment over the whole wave: the head
// carries it, the tail carries zero under the same key (the carry stream stays sorted).
__device__ __forceinline__ void wave_store_or_carry(uint32_t key, const Fr& v, bool tail, bool from0, Fr* __restrict__ out,
                                                    uint32_t* ck, Fr* cv) {
  const int lane = threadIdx.x & 63;
  if (!tail) return;
  if (from0) {
    ck[0] = key, cv[0] = v;
    if (lane == 63) ck[1] = key, cv[1] = Fr::zero();
  } else if (lane == 63) {
    ck[1] = key, cv[1] = v;
  } else if (key != SPMV_NO_KEY) {
    out[key] = v;
  }
}

}  // namespace lh
