// The hand-off between the workgroups of a round kernel - the ONE place where the prover's correctness rests on memory
// ordering between workgroups (DESIGN.md "No fence between the workgroups of a round").  Every workgroup leaves its partial
// sums (fin_put), draws a ticket from a counter that only ever grows (the host knows its value before the launch, so
// nothing has to be zeroed), and the workgroup that draws the launch's last ticket re-reads all partials (fin_get), adds
// them and publishes the result to the host - no second launch.  A round kernel ends with fin_put per sum as it reduces
// and ONE call of finish_round (a workgroup holds its sums in thread 0) or finish_round_waves (in lane 0 of one wave per
// evaluation point).  The host's half is RoundLaunch (dev.hpp).
// Read by hipcc and by the runtime compiler alike (jit.cpp: the compiled kernel includes this text), so it depends on
// ff.cuh / reduce.cuh only.
#pragma once
#include "ff.cuh"

namespace lh {

struct ScFinishArgs {
  uint32_t* ticket;      // device counter
  uint32_t last_ticket;  // value the last workgroup of this launch draws
  Fr* out_host;          // pinned
  uint32_t* flag;        // pinned
  uint32_t seq;
  // sharded rounds, all-reduce variant (Options::comm_round, comm.cpp comm_sum_publish): the sums ALSO leave as 8 u64
  // lanes each, lane = 32-bit limb | tag << SC_LANE_TAG_SHIFT - what ncclAllReduce(ncclSum, ncclUint64) adds over the ranks
  // without losing a carry; null otherwise
  uint64_t* wide;
  uint32_t tag;
  // the workgroups' partial sums on their way to the workgroup that draws the launch's last ticket, as 8-byte lanes
  // (limb | seq << 32) in a buffer that holds nothing else (Ctx::fin_lanes, fin_put / fin_get below): each lane
  // validates itself, so the hand-off needs no fence - an agent-scope release per workgroup makes the L2 of its XCD walk its
  // dirty lines, ~27 ns per workgroup of a launch that has just stored a table (tools/ubench/u32_bind.hip: a 2^24-entry
  // bind 0.147 -> 0.108 ms).  Null: the partials travel through `partials` under release / acquire fences.
  uint64_t* lanes;
};
// a lane of the all-reduce variant: bits [0, 40) the sum of <= 2^8 32-bit limbs, bits [40, 64) the sum of the ranks' tags -
// every rank stamps the same tag < 2^24 / R, so a lane whose upper bits read R * tag is the finished sum of THIS round
// (lanes are 8-byte stores: each validates itself, no flag and no ordering between them is needed)
constexpr unsigned SC_LANE_TAG_SHIFT = 40;

}  // namespace lh

#if defined(__HIPCC__)
#include "reduce.cuh"

namespace lh {

__device__ __forceinline__ void publish_flag(uint32_t* flag, uint32_t seq) {
  // results were written by this thread just before: release them to the host, then the sequence number
  __hip_atomic_store(flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// A workgroup's partial sum number idx on its way to the workgroup that finishes the launch (ScFinishArgs::lanes):
// eight self-validating 8-byte lanes when the launch has a lane buffer, a plain store (under the fences of the ticket
// - or straight into the host buffer of a single-workgroup launch, whose `partials` IS the host buffer) when not.
__device__ __forceinline__ void fin_put(const ScFinishArgs& f, Fr* partials, size_t idx, const Fr& v) {
  if (f.lanes && gridDim.x * gridDim.y > 1) {
#pragma unroll
    for (int k = 0; k < 8; k++)
      __hip_atomic_store(&f.lanes[idx * 8 + k], (uint64_t)v.l[k] | ((uint64_t)f.seq << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  } else {
    partials[idx] = v;
  }
}
// (by the finishing workgroup, after the last ticket: every lane was stored before its workgroup drew its ticket, so the
//  poll is a formality - a lane that never arrives is a bug, and ends the kernel rather than hanging the device)
__device__ __forceinline__ Fr fin_get(const ScFinishArgs& f, const Fr* partials, size_t idx) {
  if (!f.lanes) return partials[idx];
  uint64_t v[8];
  for (uint32_t spin = 0;; spin++) {  // all eight loads in flight, then the tags
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 8; k++) v[k] = __hip_atomic_load(&f.lanes[idx * 8 + k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
    for (int k = 0; k < 8; k++) ok = ok && (uint32_t)(v[k] >> 32) == f.seq;
    if (ok) break;
    if (spin > (1u << 22)) __builtin_trap();
    __builtin_amdgcn_s_sleep(1);
  }
  Fr p;
#pragma unroll
  for (int k = 0; k < 8; k++) p.l[k] = (uint32_t)v[k];
  return p;
}

// the fused bind of a round kernel that owns pair b: BIND reads the 4 entries (4b..4b+3) of the previous round's table, binds
// them with r and (`store`) stores the bound pair (2b, 2b+1) once; the first round reads the pair as it is
template <bool BIND>
__device__ __forceinline__ void load_pair(const Fr* __restrict__ in, Fr* __restrict__ out, size_t b, const Fr& r,
                                          bool store, Fr& v0, Fr& v1) {
  if (BIND) {
    const Fr* p = in + 4 * b;
    Fr e0 = p[0], e1 = p[1], e2 = p[2], e3 = p[3];
    v0 = add(mul(sub(e1, e0), r), e0);
    v1 = add(mul(sub(e3, e2), r), e2);
    if (store) {
      out[2 * b] = v0;
      out[2 * b + 1] = v1;
    }
  } else {
    v0 = in[2 * b];
    v1 = in[2 * b + 1];
  }
}

// THE ticket (cdna_hip_programming.md Guideline 16), by one lane whose wave has drained its stores: agent-scope release,
// a relaxed draw, and on the last ticket of the batch an agent-scope acquire - then every other workgroup's stores are
// visible to this CU.  Not `fenced` (the payload travels in self-validating lanes): the relaxed draw alone.
__device__ __forceinline__ bool draw_ticket(uint32_t* ticket, uint32_t last_ticket, bool fenced = true) {
  if (fenced) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  const uint32_t t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const bool last = t == last_ticket;
  if (last && fenced) {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  return last;
}
// the ticket of a workgroup whose partial sums are on their way: true for the workgroup that finishes the launch.  Every
// thread of the workgroup calls it.  The sums were stored by wave 0 - or, `every_wave_stores`, by any wave: each drains
// its stores in front of a barrier of its own.
__device__ __forceinline__ bool fin_ticket(const ScFinishArgs& f, bool every_wave_stores = false) {
  __shared__ int is_last;
  if (every_wave_stores) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
  if (threadIdx.x < 64) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's partial stores have left
    if (threadIdx.x == 0) is_last = draw_ticket(f.ticket, f.last_ticket, !f.lanes);
  }
  __syncthreads();
  return is_last != 0;
}

// by the ONE thread that publishes, once the launch's D sums are in f.out_host and visible to it (its own stores, or the
// workgroup's before a barrier).  Sharded rounds of the all-reduce variant (ScFinishArgs::wide): the sums leave a second
// time as tagged u64 lanes - re-read with agent-scope loads, the stores may be another wave's.
__device__ __forceinline__ void publish_round(const ScFinishArgs& f, int D) {
  if (f.wide) {
    for (int x = 0; x < D; x++)
      for (int k = 0; k < 8; k++) {
        const uint32_t limb = __hip_atomic_load(&f.out_host[x].l[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        f.wide[8 * x + k] = (uint64_t)limb | ((uint64_t)f.tag << SC_LANE_TAG_SHIFT);
      }
  }
  publish_flag(f.flag, f.seq);
}

// The closing step of a round kernel, WORKGROUP form: workgroup w has put its D sums at partials[w * D + x] - thread 0, or
// threads 0..D-1 of wave 0, one sum each (`PUT_BY_D_THREADS`: each releases its store to the host where the launch is a
// single workgroup, and a barrier stands in front of the publish) - and every thread calls this.  A single-workgroup
// launch's `partials` IS the host buffer: it only publishes.  lds: 4 slots of reduction scratch.
template <int D, bool PUT_BY_D_THREADS = false>
__device__ __forceinline__ void finish_round(const ScFinishArgs& f, const Fr* __restrict__ partials, Fr* lds) {
  if (gridDim.x == 1) {
    if (PUT_BY_D_THREADS) __syncthreads();
    if (threadIdx.x == 0) publish_round(f, D);
    return;
  }
  if (!fin_ticket(f)) return;
  const uint32_t blocks = gridDim.x;
#pragma unroll
  for (int x = 0; x < D; x++) {
    Fr acc = Fr::zero();
    for (uint32_t i = threadIdx.x; i < blocks; i += blockDim.x) acc = add(acc, fin_get(f, partials, (size_t)i * D + x));
    acc = block_reduce_sum(acc, lds);
    if (threadIdx.x == 0) f.out_host[x] = acc;
  }
  if (threadIdx.x == 0) publish_round(f, D);
}

// The closing step, WAVE-PER-POINT form: lane 0 of a wave has put the sum of its slot s (of `slots` in the launch) at
// point x at partials[s * D + x]; the finishing workgroup's wave w adds the slots of points w, w + waves, ...  A launch
// of one workgroup and one slot has its sums in the host buffer already; a single workgroup of several slots draws the
// one ticket like any other (RoundLaunch counts it).
__device__ __forceinline__ void finish_round_waves(const ScFinishArgs& f, const Fr* __restrict__ partials, int D, uint32_t slots) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
  if (gridDim.x * gridDim.y > 1 || slots > 1) {
    if (!fin_ticket(f, true)) return;
    for (int x = wave; x < D; x += waves) {
      Fr acc = Fr::zero();
      for (uint32_t i = lane; i < slots; i += 64) acc = add(acc, fin_get(f, partials, (size_t)i * D + x));
      acc = wave_reduce_sum(acc);
      if (lane == 0) f.out_host[x] = acc;
    }
  }
  if (lane == 0) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");  // the waves' sums, ahead of the barrier and the flag
  __syncthreads();
  if (threadIdx.x == 0) publish_round(f, D);
}

}  // namespace lh
#endif
