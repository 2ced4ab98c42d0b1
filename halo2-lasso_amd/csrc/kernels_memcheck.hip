// Device half of the read-write memory-checking argument (memcheck.cpp; tests/memcheck_ref.py): the witness of a RAM trace
// (previous-write times, final cells, the multiplicities of the time differences) and the leaves of its two GKR arguments
// with the level above them.  Streaming kernels over 32-bit columns; a leaf is three 8-multiply-add terms into a wide
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

}  // namespace lh
