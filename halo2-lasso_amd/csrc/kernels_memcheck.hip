// Device half of the read-write memory-checking argument (memcheck.cpp; tests/memcheck_ref.py): the witness of a RAM trace
// (previous-write times, final cells, the multiplicities of the time differences) and the leaves of its two GKR arguments
// with the level above them, and the replay that derives a trace's read values from its stores (a segmented scan over the
// sorted operations; tests/memcheck_segment_ref.py is the specification of the segment proofs it feeds).  Streaming kernels over 32-bit columns; a leaf is three 8-multiply-add terms into a wide
// accumulator and ONE Montgomery reduction (wide.cuh), an Fr leaves as two dwordx4.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstring>
#include "dev.hpp"
#include "ff_host.hpp"
#include "launch.cuh"
#include "wide.cuh"

namespace lh {

// ------------------------------------------------------------------ 1. the trace's witness
// The operations sorted stably by cell (skey: the addresses, sidx: the positions they came from - ascending inside a cell's
// run).  Position p whose left neighbour q is on the same cell was written at time q + 1 and must read wv[q]; the first of a
// run reads the image.  The last of a run leaves the cell's final value and time.  An address >= cells (the sort looked at the
// low bits alone, so such a key sits in some cell's run: it matches no neighbour, and indexes nothing) or a wrong read sets *bad.
__global__ __launch_bounds__(256) void memcheck_trace_kernel(const uint32_t* __restrict__ skey, const uint32_t* __restrict__ sidx,
                                                             const uint32_t* __restrict__ rv, const uint32_t* __restrict__ wv,
                                                             const uint32_t* __restrict__ init, size_t n, size_t cells,
                                                             uint32_t* __restrict__ rt, uint32_t* __restrict__ fv,
                                                             uint32_t* __restrict__ ft, uint32_t* __restrict__ bad) {
  GSTRIDE(i, n) {
    const uint32_t a = skey[i], p = sidx[i];
    if (a >= cells) {
      rt[p] = 0u;
      *bad = 1u;
      continue;
    }
    uint32_t t = 0u, want;
    if (i > 0 && skey[i - 1] == a) {
      const uint32_t q = sidx[i - 1];
      t = q + 1u, want = wv[q];
    } else {
      want = init ? init[a] : 0u;
    }
    if (rv[p] != want) *bad = 1u;
    rt[p] = t;
    if (i + 1 == n || skey[i + 1] != a) fv[a] = wv[p], ft[a] = p + 1u;
  }
}
bool k_memcheck_trace(Ctx& c, const uint32_t* addr, const uint32_t* rv, const uint32_t* wv, size_t num_vars, size_t mem_vars,
                      const uint32_t* d_init, uint32_t* rt, uint32_t* fv, uint32_t* ft) {
  LH_REQUIRE(num_vars >= 1 && num_vars < 31 && mem_vars >= 1 && mem_vars < 31, LH_ERR_ARG, "memcheck_trace: bad shape");
  LH_REQUIRE(addr && rv && wv && rt && fv && ft, LH_ERR_ARG, "memcheck_trace: null column");
  const size_t n = (size_t)1 << num_vars, cells = (size_t)1 << mem_vars;
  // algorithmic bytes: the sort reads the addresses and writes (key, position) pairs (4 + 8), the pass reads the pairs (8), gathers
  // rv[p], wv[p], wv[q] (12) and writes rt (4); the cells are pre-filled and the touched ones rewritten (2 x 8 at most)
  ProfScope ps(c, "memcheck_trace", 36.0 * n + 16.0 * cells, 0.0, (double)n);
  ArenaScope scope(c.arena);  // (everything below is queued on the ctx's stream: the next user of this memory comes behind it)
  uint32_t* skey = c.arena.alloc_n<uint32_t>(n);
  uint32_t* sidx = c.arena.alloc_n<uint32_t>(n);
  uint32_t* bad = c.arena.alloc_n<uint32_t>(1);
  LH_HIP(hipMemsetAsync(bad, 0, sizeof(uint32_t), c.stream));
  if (d_init) LH_HIP(hipMemcpyAsync(fv, d_init, cells * sizeof(uint32_t), hipMemcpyDeviceToDevice, c.stream));
  else LH_HIP(hipMemsetAsync(fv, 0, cells * sizeof(uint32_t), c.stream));
  LH_HIP(hipMemsetAsync(ft, 0, cells * sizeof(uint32_t), c.stream));
  sort_pairs_u32(c, addr, skey, nullptr, sidx, n, (unsigned)mem_vars);  // (no values given: the positions)
  hipLaunchKernelGGL(memcheck_trace_kernel, dim3(cu_grid(c, n)), dim3(256), 0, c.stream, skey, sidx, rv, wv, d_init, n, cells,
                     rt, fv, ft, bad);
  uint32_t h_bad = 0;
  c.d2h(&h_bad, bad, sizeof(uint32_t));  // the one flag readback of a proof
  return h_bad == 0;
}

// ------------------------------------------------------------------ 2. m[d] = #{i : i - rt[i] = d}
// The differences are as skewed as the trace: one hot cell makes every difference 0.  The lanes of a wave that hold the same
// difference are combined before the atomic (as the LogUp join's counts are, kernels_plonk.hip m_probe_kernel): a hot cell
// costs a wave one ballot per turn, a uniform trace at most 64 ballots per wave and atomics spread over the column.  The
// last group's count stays with the wave (pend_v, pend_c: the same in every lane) and is added only when another difference
// follows it, so a wave whose lanes all hold one difference turn after turn - the hot cell - issues ONE atomic in all, not
// one per turn (2^24 operations on one cell: 2^18 atomics on one word took 3.0 ms).  Every turn of the loop is
// taken by whole workgroups, so the ballots see whole waves.
__global__ __launch_bounds__(256) void memcheck_m_kernel(const uint32_t* __restrict__ rt, size_t n, uint32_t* __restrict__ m) {
  const int lane = (int)(threadIdx.x & 63);
  uint32_t pend_v = 0u, pend_c = 0u;
  for (size_t base = (size_t)blockIdx.x * blockDim.x; base < n; base += (size_t)gridDim.x * blockDim.x) {
    const size_t i = base + threadIdx.x;
    uint32_t d = 0xffffffffu;
    if (i < n) d = (uint32_t)i - rt[i];
    const bool live = d < n;  // (rt[i] <= i by construction; a difference outside the column is dropped, never added)
    unsigned long long todo = __ballot(live);
    while (todo) {
      const int leader = __ffsll((long long)todo) - 1;
      const uint32_t v = __shfl(d, leader, 64);
      const unsigned long long same = __ballot(live && d == v) & todo;
      const uint32_t count = (uint32_t)__popcll(same);
      if (pend_c && v == pend_v) {
        pend_c += count;
      } else {
        if (pend_c && lane == 0) atomicAdd(&m[pend_v], pend_c);
        pend_v = v, pend_c = count;
      }
      todo &= ~same;
    }
  }
  if (pend_c && lane == 0) atomicAdd(&m[pend_v], pend_c);
}
void k_memcheck_m(Ctx& c, const uint32_t* rt, size_t n, uint32_t* m) {
  LH_REQUIRE(rt && m && n >= 1 && n < ((size_t)1 << 32), LH_ERR_ARG, "memcheck_m: bad shape");
  // 4 n read, 4 n cleared, at most 4 n added
  ProfScope ps(c, "memcheck_m", 12.0 * n, 0.0, (double)n);
  LH_HIP(hipMemsetAsync(m, 0, n * sizeof(uint32_t), c.stream));
  hipLaunchKernelGGL(memcheck_m_kernel, dim3(cu_grid(c, n)), dim3(256), 0, c.stream, rt, n, m);
}

// ------------------------------------------------------------------ 3. memory leaves (+ the level above), both sides in one launch
// blockIdx.y = 0: RS[i] = h(addr, rv, rt), WS[i] = h(addr, wv, i + 1) over the operations;
// blockIdx.y = 1: Init[a] = h(a, init[a], 0), Final[a] = h(a, fv[a], ft[a]) over the cells;  h(a, v, t) = a g^2 + v g + t - tau.
// The pattern of lasso_rw_leaves_batch_kernel (kernels_poly.hip): a workgroup takes tiles of 1024 leaves; VEC reads the side's
// u32 columns 16 bytes per lane into LDS and every lane then takes the leaves tile + 256 k + lane, k < 4, so that the 32-byte
// leaves of a wave leave as whole lines; !VEC (fewer than 4 leaves, or a column that is not 16-byte aligned) reads 4 bytes per
// lane.  UP (per side): `count` is half the side's leaves and the lane that makes leaves i and i + count makes their products.
// The two leaves of an index share their address term: 5 multiply-add terms and two reductions per pair of leaves.
template <bool UP, bool VEC>
__device__ __forceinline__ void memcheck_leaves_side(const MemcheckLeaves& p, const unsigned side, uint32_t (*tile)[4][1024],
                                                     const Fr& gamma_r, const Fr& gamma2_r, const Fr& one_r, const Fr& tau) {
  constexpr int SEG = UP ? 2 : 1;
  const uint32_t* const cols[4] = {p.col[side][0], p.col[side][1], p.col[side][2], p.col[side][3]};
  Fr* const leaf0 = p.leaf[side][0];
  Fr* const leaf1 = p.leaf[side][1];
  const size_t count = p.count[side];
  const size_t tiles = (count + 1023) / 1024;
  for (size_t t = blockIdx.x; t < tiles; t += gridDim.x) {  // (uniform per workgroup: the barriers below are reached by all)
    const size_t base = t * 1024;
    if (VEC) {
      const size_t q = base + 4 * (size_t)threadIdx.x;  // (count is a multiple of 4: q + 3 < count)
      if (q < count) {
#pragma unroll
        for (int s = 0; s < SEG; s++)
#pragma unroll
          for (int k = 0; k < 4; k++)
            if (cols[k])
              *reinterpret_cast<uint4*>(&tile[s][k][4 * threadIdx.x]) = *reinterpret_cast<const uint4*>(cols[k] + s * count + q);
      }
      __syncthreads();
    }
#pragma unroll 1
    for (int k = 0; k < 4; k++) {
      const size_t i = base + 256 * (size_t)k + threadIdx.x;
      if (i >= count) break;
      Fr h0[SEG], h1[SEG];
#pragma unroll
      for (int s = 0; s < SEG; s++) {
        const size_t j = i + s * count;
        const uint32_t at = 256 * k + threadIdx.x;
        uint32_t x[4];
#pragma unroll
        for (int q = 0; q < 4; q++) x[q] = cols[q] ? (VEC ? tile[s][q][at] : cols[q][j]) : 0u;
        // side 0: addr, rv, rt, wv and the time j + 1; side 1: the cell j, init, time 0, fv, ft
        const uint32_t a = side ? (uint32_t)j : x[0], v0 = side ? x[0] : x[1], t0 = side ? 0u : x[2];
        const uint32_t v1 = side ? x[1] : x[3], t1 = side ? x[2] : (uint32_t)j + 1u;
        Wide w0 = Wide::zero();
        wide_mac(w0, gamma2_r, a);
        Wide w1 = w0;
        wide_mac(w0, gamma_r, v0);
        if (!side) wide_mac(w0, one_r, t0);
        wide_mac(w1, gamma_r, v1);
        wide_mac(w1, one_r, t1);
        h0[s] = sub(wide_redc(w0), tau);
        h1[s] = sub(wide_redc(w1), tau);
        leaf0[j] = h0[s];
        leaf1[j] = h1[s];
      }
      if (UP) {
        p.up[side][0][i] = mul(h0[0], h0[SEG - 1]);
        p.up[side][1][i] = mul(h1[0], h1[SEG - 1]);
      }
    }
    if (VEC) __syncthreads();  // (the tile is overwritten by the next turn)
  }
}
template <bool VEC>
__global__ __launch_bounds__(256) void memcheck_leaves_kernel(MemcheckLeaves p, Fr gamma_r, Fr gamma2_r, Fr one_r, Fr tau) {
  __shared__ __align__(16) uint32_t tile[2][4][1024];
  const unsigned side = blockIdx.y;
  if (p.up[side][0]) memcheck_leaves_side<true, VEC>(p, side, tile, gamma_r, gamma2_r, one_r, tau);
  else memcheck_leaves_side<false, VEC>(p, side, tile, gamma_r, gamma2_r, one_r, tau);
}
void k_memcheck_leaves(Ctx& c, const MemcheckLeaves& a, size_t num_vars, size_t mem_vars, const Fr& gamma, const Fr& gamma2,
                       const Fr& tau) {
  LH_REQUIRE(num_vars >= 1 && num_vars < 31 && mem_vars >= 1 && mem_vars < 31, LH_ERR_ARG, "memcheck_leaves: bad shape");
  MemcheckLeaves p = a;
  const size_t len[2] = {(size_t)1 << num_vars, (size_t)1 << mem_vars};
  bool vec = true;
  double bytes = 0;
  size_t tiles = 1;
  for (int side = 0; side < 2; side++) {
    const bool up = p.up[side][0] != nullptr;
    LH_REQUIRE(p.leaf[side][0] && p.leaf[side][1] && (!up || p.up[side][1]), LH_ERR_ARG, "memcheck_leaves: null leaf table");
    p.count[side] = up ? len[side] / 2 : len[side];
    vec = vec && p.count[side] % 4 == 0;
    int ncols = 0;
    for (int k = 0; k < 4; k++) {
      // side 0: addr, rv, rt, wv; side 1: init (null: an all-zero image), fv, ft
      const bool optional = side == 1 && k == 0, unused = side == 1 && k == 3;
      LH_REQUIRE(unused ? p.col[side][k] == nullptr : optional || p.col[side][k] != nullptr, LH_ERR_ARG,
                 "memcheck_leaves: null column");
      vec = vec && (uintptr_t)p.col[side][k] % 16 == 0;
      ncols += p.col[side][k] != nullptr;
    }
    bytes += (4.0 * ncols + 64.0 + (up ? 32.0 : 0.0)) * len[side];
    tiles = std::max(tiles, (p.count[side] + 1023) / 1024);
  }
  // per operation 16 B read and two leaves (64 B) written, per cell 12 B (8 without an image) and 64 B; + 32 B with the level above
  ProfScope ps(c, "memcheck_leaves", bytes, 6.0 * (len[0] + len[1]), (double)(len[0] + len[1]));
  const dim3 grid(cu_grid(c, tiles, 1), 2u);
  const Fr g1 = prescale_r(gamma), g2 = prescale_r(gamma2), o1 = prescale_r(Fr::one());
  if (vec) hipLaunchKernelGGL(memcheck_leaves_kernel<true>, grid, dim3(256), 0, c.stream, p, g1, g2, o1, tau);
  else hipLaunchKernelGGL(memcheck_leaves_kernel<false>, grid, dim3(256), 0, c.stream, p, g1, g2, o1, tau);
}

// ------------------------------------------------------------------ 4. range leaves (+ the level above) of the two fractions
// Lane i < half makes the leaves i and i + half - the pair Layer::up joins - of BOTH fractions, which share the index:
//   fraction 0: p == 1 (the shared table of ones), q = delta + (i - rt[i]);   node = (q_l + q_r, q_l q_r)
//   fraction 1: p = -m[i],                         q = delta + i;             node = (p_l q_r + p_r q_l, q_l q_r)
// 8 B read per index; six tables and the ones written (7 x 32 B per index), four half-size ones with UP (2 x 32 B per index).
template <bool UP>
__global__ __launch_bounds__(256) void memcheck_range_leaves_kernel(MemcheckRangeLeaves a, size_t half, Fr delta, Fr one_r) {
  const Fr one = Fr::one();
  GSTRIDE(i, half) {
    Fr q0[2], p1[2], q1[2];
#pragma unroll
    for (int s = 0; s < 2; s++) {
      const size_t j = i + (s ? half : 0);
      q0[s] = add(delta, wide_small(one_r, (uint32_t)j - a.rt[j]));
      p1[s] = neg(wide_small(one_r, a.m[j]));
      q1[s] = add(delta, wide_small(one_r, (uint32_t)j));
      a.ones[j] = one;
      a.q0[j] = q0[s];
      a.p1[j] = p1[s];
      a.q1[j] = q1[s];
    }
    if (UP) {
      a.p0_up[i] = add(q0[0], q0[1]);
      a.q0_up[i] = mul(q0[0], q0[1]);
      a.p1_up[i] = add(mul(p1[0], q1[1]), mul(p1[1], q1[0]));
      a.q1_up[i] = mul(q1[0], q1[1]);
    }
  }
}
void k_memcheck_range_leaves(Ctx& c, const MemcheckRangeLeaves& a, size_t num_vars, bool up, const Fr& delta) {
  LH_REQUIRE(num_vars >= 1 && num_vars < 31, LH_ERR_ARG, "memcheck_range_leaves: bad shape");
  LH_REQUIRE(a.rt && a.m && a.ones && a.q0 && a.p1 && a.q1 && (!up || (a.p0_up && a.q0_up && a.p1_up && a.q1_up)), LH_ERR_ARG,
             "memcheck_range_leaves: null column");
  const size_t half = (size_t)1 << (num_vars - 1);
  ProfScope ps(c, "memcheck_range_leaves", (2 * (8.0 + 4 * 32.0) + (up ? 4 * 32.0 : 0.0)) * half, (up ? 4.0 : 0.0) * half,
               (double)(2 * half));
  const Fr o1 = prescale_r(Fr::one());
  if (up) hipLaunchKernelGGL(memcheck_range_leaves_kernel<true>, dim3(cu_grid(c, half)), dim3(256), 0, c.stream, a, half, delta, o1);
  else hipLaunchKernelGGL(memcheck_range_leaves_kernel<false>, dim3(cu_grid(c, half)), dim3(256), 0, c.stream, a, half, delta, o1);
}

// ------------------------------------------------------------------ 5. the replay: read values from stores (lh_memcheck_replay)
// The operations sorted stably by cell, as for the witness above.  The value an operation reads is an EXCLUSIVE SEGMENTED SCAN
// over the sorted order: segments are the runs of one address, the operator is "the right operand wins if it is a store", the
// identity the cell's image word.  What the scan carries over a range of sorted operations is a ReplayState: the key of the
// range's last segment, whether that segment holds a store inside the range (HAS) and the last such store's word, and whether
// the range is ONE segment (SPAN) - a range that is SPAN and not HAS is transparent: joined to the right of another state of
// the same key it changes nothing, so a carry passes through any number of store-free tiles of a hot cell.
//
// The shape of spartan_spmv (spmv.cuh): a workgroup of 256 lanes takes a tile of REPLAY_TILE sorted operations, lane t the run
// of REPLAY_RUN consecutive ones from 8 t; the lanes' states are scanned over wave shuffles, the four waves' ends joined in
// LDS.  An operation whose value the tile knows - an earlier store of its segment inside the tile, or a segment that begins
// inside the tile - is written at once: rv[p], wv[p] scattered to its position p, final[a] by the last operation of a segment.
// The others are OPEN: the leading operations of the tile's first segment up to and including its first store, open_len of
// them.  memcheck_replay_carry_kernel scans the tiles' states (one workgroup, the same block scan, 2048 tiles per turn) and
// memcheck_replay_open_kernel writes the open operations from their tile's carry.  No atomics; every word is written once.
// An address >= cells sets *bad and reads no image word and writes no final cell (its positions p are in range: rv, wv).
constexpr int REPLAY_RUN = 8;
constexpr int REPLAY_TILE = 256 * REPLAY_RUN;
static_assert(REPLAY_TILE <= 4096, "tests/test_gpu_memcheck_replay.py places its stores around tiles of at most 4096");
enum : uint32_t { RP_HAS = 1u, RP_SPAN = 2u, RP_EMPTY = 4u };
struct ReplayState {
  uint32_t key, val, flags;
};
__device__ __forceinline__ ReplayState replay_empty() { return ReplayState{0u, 0u, RP_EMPTY}; }
__device__ __forceinline__ ReplayState replay_item(uint32_t key, bool store, uint32_t val) {
  return ReplayState{key, val, RP_SPAN | (store ? RP_HAS : 0u)};
}
// (by value and select by select on the words: a choice between the two states as objects goes through scratch)
__device__ __forceinline__ ReplayState replay_join(const ReplayState l, const ReplayState r) {
  // r goes on with l's last segment and ends in it; else r's last segment begins inside r, or at its first operation
  const bool on = (r.flags & RP_SPAN) && r.key == l.key;
  uint32_t key = r.key;
  uint32_t val = on && !(r.flags & RP_HAS) ? l.val : r.val;
  uint32_t flags = on ? (l.flags & (RP_HAS | RP_SPAN)) | (r.flags & RP_HAS) : r.flags & RP_HAS;
  if (l.flags & RP_EMPTY) val = r.val, flags = r.flags;
  if (r.flags & RP_EMPTY) key = l.key, val = l.val, flags = l.flags;
  return ReplayState{key, val, flags};
}
__device__ __forceinline__ ReplayState replay_shfl_up(const ReplayState& s, int off) {
  return ReplayState{__shfl_up(s.key, off, 64), __shfl_up(s.val, off, 64), __shfl_up(s.flags, off, 64)};
}
__device__ __forceinline__ uint4 replay_pack(const ReplayState& s) { return make_uint4(s.key, s.val, s.flags, 0u); }
__device__ __forceinline__ ReplayState replay_unpack(const uint4& u) { return ReplayState{u.x, u.y, u.z}; }
// The state of everything the lanes below this one hold (EMPTY for lane 0 of the workgroup), *total: of all 256 lanes.
// Reached by whole workgroups (two barriers); `ends` - the four waves' ends, field by field - is free again on return.
__device__ __forceinline__ ReplayState replay_block_scan(ReplayState s, uint32_t (*ends)[4], ReplayState* total) {
  const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const ReplayState o = replay_shfl_up(s, off);
    if (lane >= off) s = replay_join(o, s);
  }
  ReplayState x = replay_shfl_up(s, 1);
  if (lane == 0) x.key = 0u, x.val = 0u, x.flags = RP_EMPTY;
  if (lane == 63) ends[0][wave] = s.key, ends[1][wave] = s.val, ends[2][wave] = s.flags;
  __syncthreads();
  ReplayState before = replay_empty(), all = replay_empty();
#pragma unroll
  for (int w = 0; w < 4; w++) {
    const ReplayState e = {ends[0][w], ends[1][w], ends[2][w]};
    if (w < wave) before = replay_join(before, e);
    all = replay_join(all, e);
  }
  __syncthreads();
  *total = all;
  return replay_join(before, x);
}
// what an operation on cell `key` reads, given the state of everything before it in the scanned range: the last store's
// word (true), or nothing known (false: the identity, or - open - the range's carry)
__device__ __forceinline__ bool replay_hit(const ReplayState& x, uint32_t key) {
  return !(x.flags & RP_EMPTY) && x.key == key && (x.flags & RP_HAS);
}
__device__ __forceinline__ bool replay_open(const ReplayState& x, uint32_t key) {
  return (x.flags & RP_EMPTY) || (x.key == key && (x.flags & (RP_HAS | RP_SPAN)) == RP_SPAN);
}

__global__ __launch_bounds__(256) void memcheck_replay_tile_kernel(
    const uint32_t* __restrict__ skey, const uint32_t* __restrict__ sidx, const uint32_t* __restrict__ store,
    const uint32_t* __restrict__ val, const uint32_t* __restrict__ image, size_t n, size_t cells, size_t tiles,
    uint32_t* __restrict__ rv, uint32_t* __restrict__ wv, uint32_t* __restrict__ fin, uint4* __restrict__ tile_state,
    uint32_t* __restrict__ open_len, uint32_t* __restrict__ bad) {
  __shared__ uint32_t ends[3][4];
  __shared__ uint32_t opens[4];
  const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
  for (size_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {  // (uniform per workgroup: the barriers are reached by all)
    const size_t i0 = tile * REPLAY_TILE + (size_t)threadIdx.x * REPLAY_RUN;
    uint32_t a[REPLAY_RUN], p[REPLAY_RUN], v[REPLAY_RUN], st[REPLAY_RUN];
    if (i0 + REPLAY_RUN <= n) {  // (the arena's blocks are 256-byte aligned, a run's offset 32-byte)
#pragma unroll
      for (int k = 0; k < REPLAY_RUN; k += 4) {
        const uint4 ka = *reinterpret_cast<const uint4*>(skey + i0 + k), kp = *reinterpret_cast<const uint4*>(sidx + i0 + k);
        a[k] = ka.x, a[k + 1] = ka.y, a[k + 2] = ka.z, a[k + 3] = ka.w;
        p[k] = kp.x, p[k + 1] = kp.y, p[k + 2] = kp.z, p[k + 3] = kp.w;
      }
    } else {  // (past the end: dead operations behind every live one - they are before nobody, and write nothing)
#pragma unroll
      for (int k = 0; k < REPLAY_RUN; k++) {
        const bool live = i0 + k < n;
        a[k] = live ? skey[i0 + k] : 0u, p[k] = live ? sidx[i0 + k] : 0u;
      }
    }
#pragma unroll
    for (int k = 0; k < REPLAY_RUN; k++) {
      const bool live = i0 + k < n;
      st[k] = live ? store[p[k]] : 0u;
      v[k] = live ? val[p[k]] : 0u;
    }
    const uint32_t next = i0 + REPLAY_RUN < n ? skey[i0 + REPLAY_RUN] : 0u;  // (read only where there is a next operation)
    ReplayState s = replay_empty();
#pragma unroll
    for (int k = 0; k < REPLAY_RUN; k++) s = replay_join(s, replay_item(a[k], st[k] != 0u, v[k]));
    ReplayState total;
    ReplayState x = replay_block_scan(s, ends, &total);
    uint32_t nopen = 0u;
#pragma unroll
    for (int k = 0; k < REPLAY_RUN; k++) {
      const size_t i = i0 + k;
      if (i < n) {
        const bool inside = a[k] < cells;
        if (!inside) *bad = 1u;
        if (replay_open(x, a[k])) {
          nopen++;
        } else {
          const uint32_t r = replay_hit(x, a[k]) ? x.val : (inside && image ? image[a[k]] : 0u);
          const uint32_t w = st[k] ? v[k] : r;
          rv[p[k]] = r, wv[p[k]] = w;
          const uint32_t after = k + 1 < REPLAY_RUN ? a[(k + 1) % REPLAY_RUN] : next;
          const bool last = i + 1 == n || after != a[k];
          if (last && inside && fin) fin[a[k]] = w;
        }
      }
      x = replay_join(x, replay_item(a[k], st[k] != 0u, v[k]));
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) nopen += __shfl_xor(nopen, off, 64);
    if (lane == 0) opens[wave] = nopen;
    __syncthreads();
    if (threadIdx.x == 0) {
      open_len[tile] = opens[0] + opens[1] + opens[2] + opens[3];
      tile_state[tile] = replay_pack(total);
    }
    __syncthreads();  // (opens is overwritten by the next turn)
  }
}
// carry[t] = the state of every operation before tile t (EMPTY for tile 0): one workgroup, REPLAY_TILE tiles per turn
__global__ __launch_bounds__(256) void memcheck_replay_carry_kernel(const uint4* __restrict__ tile_state, size_t tiles,
                                                                    uint4* __restrict__ carry) {
  __shared__ uint32_t ends[3][4];
  ReplayState run = replay_empty();
  for (size_t base = 0; base < tiles; base += REPLAY_TILE) {
    const size_t t0 = base + (size_t)threadIdx.x * REPLAY_RUN;
    uint32_t sk[REPLAY_RUN], sv[REPLAY_RUN], sf[REPLAY_RUN];
    ReplayState agg = replay_empty();
#pragma unroll
    for (int k = 0; k < REPLAY_RUN; k++) {
      sk[k] = 0u, sv[k] = 0u, sf[k] = RP_EMPTY;  // (past the last tile)
      if (t0 + k < tiles) {
        const uint4 u = tile_state[t0 + k];
        sk[k] = u.x, sv[k] = u.y, sf[k] = u.z;
      }
      agg = replay_join(agg, ReplayState{sk[k], sv[k], sf[k]});
    }
    ReplayState total;
    ReplayState x = replay_join(run, replay_block_scan(agg, ends, &total));
#pragma unroll
    for (int k = 0; k < REPLAY_RUN; k++) {
      if (t0 + k < tiles) carry[t0 + k] = replay_pack(x);
      x = replay_join(x, ReplayState{sk[k], sv[k], sf[k]});
    }
    run = replay_join(run, total);
  }
}
// the open operations of every tile: all on the tile's first cell, all loads but perhaps the last one
__global__ __launch_bounds__(256) void memcheck_replay_open_kernel(
    const uint32_t* __restrict__ skey, const uint32_t* __restrict__ sidx, const uint32_t* __restrict__ store,
    const uint32_t* __restrict__ val, const uint32_t* __restrict__ image, size_t n, size_t cells, size_t tiles,
    const uint4* __restrict__ carry, const uint32_t* __restrict__ open_len, uint32_t* __restrict__ rv, uint32_t* __restrict__ wv,
    uint32_t* __restrict__ fin) {
  for (size_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const size_t base = tile * REPLAY_TILE;
    const uint32_t a = skey[base], len = open_len[tile];
    const bool inside = a < cells;
    const ReplayState c = replay_unpack(carry[tile]);
    const uint32_t r = replay_hit(c, a) ? c.val : (inside && image ? image[a] : 0u);
    for (uint32_t j = threadIdx.x; j < len; j += blockDim.x) {
      const size_t i = base + j;
      const uint32_t p = sidx[i];
      const uint32_t w = store[p] != 0u ? val[p] : r;
      rv[p] = r, wv[p] = w;
      if (fin && inside && (i + 1 == n || skey[i + 1] != a)) fin[a] = w;
    }
  }
}
bool k_memcheck_replay(Ctx& c, const uint32_t* addr, const uint32_t* store, const uint32_t* val, size_t num_vars, size_t mem_vars,
                       const uint32_t* d_image, uint32_t* rv, uint32_t* wv, uint32_t* fin) {
  LH_REQUIRE(num_vars >= 1 && num_vars < 31 && mem_vars >= 1 && mem_vars < 31, LH_ERR_ARG, "memcheck_replay: bad shape");
  LH_REQUIRE(addr && store && val && rv && wv, LH_ERR_ARG, "memcheck_replay: null column");
  const size_t n = (size_t)1 << num_vars, cells = (size_t)1 << mem_vars, tiles = (n + REPLAY_TILE - 1) / REPLAY_TILE;
  // algorithmic bytes: the sort reads the addresses and writes (key, position) pairs (4 + 8), the scan reads the pairs (8), gathers
  // store[p], val[p] (8) and scatters rv[p], wv[p] (8); the final cells are pre-filled (read 4 with an image, write 4) and the
  // touched ones rewritten (4).  (Not counted: 32 B per tile of states and carries, the second visit of the open operations.)
  ProfScope ps(c, "memcheck_replay", 36.0 * n + (fin ? (d_image ? 12.0 : 8.0) * cells : 0.0), 0.0, (double)n);
  ArenaScope scope(c.arena);  // (everything below is queued on the ctx's stream: the next user of this memory comes behind it)
  uint32_t* skey = c.arena.alloc_n<uint32_t>(n);
  uint32_t* sidx = c.arena.alloc_n<uint32_t>(n);
  uint4* tile_state = c.arena.alloc_n<uint4>(tiles);
  uint4* carry = c.arena.alloc_n<uint4>(tiles);
  uint32_t* open_len = c.arena.alloc_n<uint32_t>(tiles);
  uint32_t* bad = c.arena.alloc_n<uint32_t>(1);
  LH_HIP(hipMemsetAsync(bad, 0, sizeof(uint32_t), c.stream));
  if (fin) {
    if (d_image) LH_HIP(hipMemcpyAsync(fin, d_image, cells * sizeof(uint32_t), hipMemcpyDeviceToDevice, c.stream));
    else LH_HIP(hipMemsetAsync(fin, 0, cells * sizeof(uint32_t), c.stream));
  }
  sort_pairs_u32(c, addr, skey, nullptr, sidx, n, (unsigned)mem_vars);  // (no values given: the positions)
  const unsigned grid = cu_grid(c, tiles, 1);
  hipLaunchKernelGGL(memcheck_replay_tile_kernel, dim3(grid), dim3(256), 0, c.stream, skey, sidx, store, val, d_image, n, cells,
                     tiles, rv, wv, fin, tile_state, open_len, bad);
  hipLaunchKernelGGL(memcheck_replay_carry_kernel, dim3(1), dim3(256), 0, c.stream, tile_state, tiles, carry);
  hipLaunchKernelGGL(memcheck_replay_open_kernel, dim3(grid), dim3(256), 0, c.stream, skey, sidx, store, val, d_image, n, cells,
                     tiles, carry, open_len, rv, wv, fin);
  uint32_t h_bad = 0;
  c.d2h(&h_bad, bad, sizeof(uint32_t));  // the one flag readback
  return h_bad == 0;
}

}  // namespace lh
