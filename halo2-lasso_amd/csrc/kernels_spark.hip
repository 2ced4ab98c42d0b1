// Device half of Spark (spark.cpp; tests/spark_ref.py): the memories of an opening - gathers of field elements from the eq
// tables of the verifier's point by the committed u32 index columns - with the claimed value, and the leaves of the
// memory-checking product trees over those memories.  Unlike every other leaf kernel here the memory VALUES are field
// elements (eq(r_j, .) is fixed by the point, not a registered table of words): a leaf costs one full product E gamma; its
// small terms (index gamma^2 + counter) go through the wide accumulator and one reduction (wide.cuh).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstring>
#include "dev.hpp"
#include "ff_host.hpp"
#include "launch.cuh"
#include "reduce.cuh"
#include "wide.cuh"

namespace lh {

// ------------------------------------------------------------------ 1. E_j = T_j[dim_j] and v = sum val prod_j E_j
// A lane takes entry k of ALL dimensions: C index loads (4 B, coalesced), C gathers of 32 B (two dwordx4 of one aligned
// 32-byte sector each), C stores of 32 B (whole lines per wave), val[k] once and C products.  The gathers are what bounds
// it: a table of 2^l * 32 B is hit at random.  The index is masked to the table: nothing is read out of
// bounds whatever the column holds (spark_commit has checked the range; the debug entry checks it too).
template <int C>
__global__ __launch_bounds__(256) void spark_e_kernel(SparkE p, size_t n, uint32_t mask, Fr* __restrict__ partial) {
  __shared__ Fr lds[4];
  Fr acc = Fr::zero();
  for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (size_t)gridDim.x * blockDim.x) {
    Fr prod = p.val[k];
#pragma unroll
    for (int j = 0; j < C; j++) {
      const Fr e = p.T[j][p.dim[j][k] & mask];
      p.E[j][k] = e;
      prod = mul(prod, e);
    }
    acc = add(acc, prod);
  }
  acc = block_reduce_sum(acc, lds);
  if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}
// one workgroup: the partial sums in a fixed order (lane t takes t, t + 256, ..), then the workgroup's tree
__global__ __launch_bounds__(256) void spark_e_sum_kernel(const Fr* __restrict__ partial, unsigned count, Fr* __restrict__ out) {
  __shared__ Fr lds[4];
  Fr acc = Fr::zero();
  for (unsigned i = threadIdx.x; i < count; i += blockDim.x) acc = add(acc, partial[i]);
  acc = block_reduce_sum(acc, lds);
  if (threadIdx.x == 0) *out = acc;
}
void k_spark_e(Ctx& c, const SparkE& p, size_t num_dims, size_t n, size_t dim_vars, Fr* out_value) {
  LH_REQUIRE(num_dims >= 1 && num_dims <= (size_t)SPARK_MAX_DIMS && n >= 1 && dim_vars >= 1 && dim_vars < 32, LH_ERR_ARG,
             "spark_e: bad shape");
  LH_REQUIRE(p.val && out_value, LH_ERR_ARG, "spark_e: null column");
  for (size_t j = 0; j < num_dims; j++) LH_REQUIRE(p.dim[j] && p.T[j] && p.E[j], LH_ERR_ARG, "spark_e: null column");
  // per entry: val (32 B), per dimension an index (4 B), a gathered element (32 B) and a stored one (32 B)
  ProfScope ps(c, "spark_e", (32.0 + 68.0 * num_dims) * n, (double)(num_dims * n), (double)n);
  ArenaScope scope(c.arena);
  const unsigned grid = cu_grid(c, n);
  Fr* partial = c.arena.alloc_n<Fr>(grid + 1);
  const uint32_t mask = (uint32_t)(((uint64_t)1 << dim_vars) - 1);
  if (num_dims == 1) hipLaunchKernelGGL(spark_e_kernel<1>, dim3(grid), dim3(256), 0, c.stream, p, n, mask, partial);
  else if (num_dims == 2) hipLaunchKernelGGL(spark_e_kernel<2>, dim3(grid), dim3(256), 0, c.stream, p, n, mask, partial);
  else hipLaunchKernelGGL(spark_e_kernel<3>, dim3(grid), dim3(256), 0, c.stream, p, n, mask, partial);
  hipLaunchKernelGGL(spark_e_sum_kernel, dim3(1), dim3(256), 0, c.stream, partial, grid, partial + grid);
  c.d2h(out_value, partial + grid, sizeof(Fr));
}

// ------------------------------------------------------------------ 2. the leaves (+ the level above), sides and dimensions in one launch
// blockIdx.y = side * C + j.  UP: `count` is half the side's leaves and the lane that makes leaves i and i + count makes
// their products too (the pair Layer::up joins).  A leaf: index gamma^2 (+ counter) as 8-multiply-add terms into the wide
// accumulator and one reduction, plus the full product value * gamma - 2 Montgomery reductions per leaf where the u32 leaf
// kernels pay one; the write leaf is the read leaf + 1, the final leaf the initial one + its counter.  Index columns are
// read 4 bytes per lane (coalesced; any alignment), field elements 32 bytes per lane: a wave's leaves leave as whole lines.
template <bool UP>
__device__ __forceinline__ void spark_leaves_side(const SparkLeaves& p, const unsigned side, const unsigned j, const size_t count,
                                                  const Fr& gamma, const Fr& gamma2_r, const Fr& one_r, const Fr& tau) {
  constexpr int SEG = UP ? 2 : 1;
  const uint32_t* const idx = side ? nullptr : p.dim[j];
  const uint32_t* const cnt = side ? p.fcs[j] : p.rts[j];
  const Fr* const mem = side ? p.T[j] : p.E[j];
  Fr* const leaf0 = side ? p.init[j] : p.rs[j];
  Fr* const leaf1 = side ? p.fin[j] : p.ws[j];  // (null: the write leaves are not stored)
  Fr* const up0 = side ? p.init_up[j] : p.rs_up[j];
  Fr* const up1 = side ? p.fin_up[j] : p.ws_up[j];
  const Fr one = Fr::one();
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) {
    Fr h0[SEG], h1[SEG];
#pragma unroll
    for (int s = 0; s < SEG; s++) {
      const size_t k = i + s * count;
      const uint32_t a = side ? (uint32_t)k : idx[k], t = cnt[k];
      Wide w = Wide::zero();
      wide_mac(w, gamma2_r, a);
      if (!side) wide_mac(w, one_r, t);
      // side 0: h(dim, E, read_ts); side 1: h(m, T[m], 0)
      h0[s] = sub(add(wide_redc(w), mul(mem[k], gamma)), tau);
      if (side) {
        Wide f = Wide::zero();
        wide_mac(f, one_r, t);
        h1[s] = add(h0[s], wide_redc(f));
      } else {
        h1[s] = add(h0[s], one);
      }
      leaf0[k] = h0[s];
      if (leaf1) leaf1[k] = h1[s];
    }
    if (UP) {
      up0[i] = mul(h0[0], h0[SEG - 1]);
      up1[i] = mul(h1[0], h1[SEG - 1]);
    }
  }
}
__global__ __launch_bounds__(256) void spark_leaves_kernel(SparkLeaves p, unsigned num_dims, size_t n, size_t cells, bool up_n,
                                                           bool up_l, Fr gamma, Fr gamma2_r, Fr one_r, Fr tau) {
  const unsigned side = blockIdx.y / num_dims, j = blockIdx.y % num_dims;
  const size_t len = side ? cells : n;
  if (side ? up_l : up_n) spark_leaves_side<true>(p, side, j, len / 2, gamma, gamma2_r, one_r, tau);
  else spark_leaves_side<false>(p, side, j, len, gamma, gamma2_r, one_r, tau);
}
void k_spark_leaves(Ctx& c, const SparkLeaves& p, size_t num_dims, size_t n, size_t dim_vars, bool up_n, bool up_l,
                    const Fr& gamma, const Fr& gamma2, const Fr& tau) {
  LH_REQUIRE(num_dims >= 1 && num_dims <= (size_t)SPARK_MAX_DIMS && n >= 2 && dim_vars >= 1 && dim_vars < 32, LH_ERR_ARG,
             "spark_leaves: bad shape");
  const size_t cells = (size_t)1 << dim_vars;
  size_t ws_stored = 0;
  for (size_t j = 0; j < num_dims; j++) {
    LH_REQUIRE(p.dim[j] && p.rts[j] && p.fcs[j] && p.E[j] && p.T[j], LH_ERR_ARG, "spark_leaves: null column");
    LH_REQUIRE(p.rs[j] && p.init[j] && p.fin[j], LH_ERR_ARG, "spark_leaves: null leaf table");
    LH_REQUIRE(!up_n || (p.rs_up[j] && p.ws_up[j]), LH_ERR_ARG, "spark_leaves: null level above the leaves");
    LH_REQUIRE(!up_l || (p.init_up[j] && p.fin_up[j]), LH_ERR_ARG, "spark_leaves: null level above the leaves");
    LH_REQUIRE(p.ws[j] || up_n, LH_ERR_ARG, "spark_leaves: write leaves neither stored nor joined");
    ws_stored += p.ws[j] != nullptr;
  }
  // per entry and dimension 8 B of columns and the memory value (32 B) read, the read leaf (32 B) written, the write leaf
  // where it is stored, 64 B of the level above; per cell 4 B and the table entry (32 B) read, two leaves (64 B) written, + 64 B / 2
  const double bytes = ((8.0 + 32.0 + 32.0 + (up_n ? 32.0 : 0.0)) * num_dims + 32.0 * ws_stored) * n +
                       (4.0 + 32.0 + 64.0 + (up_l ? 32.0 : 0.0)) * num_dims * cells;
  const double muls = (1.0 + (up_n ? 1.0 : 0.0)) * num_dims * n + (1.0 + (up_l ? 1.0 : 0.0)) * num_dims * cells;
  ProfScope ps(c, "spark_leaves", bytes, muls, (double)(num_dims * (n + cells)));
  const size_t most = std::max(up_n ? n / 2 : n, up_l ? cells / 2 : cells);
  const dim3 grid(cu_grid(c, most), (unsigned)(2 * num_dims));
  hipLaunchKernelGGL(spark_leaves_kernel, grid, dim3(256), 0, c.stream, p, (unsigned)num_dims, n, cells, up_n, up_l, gamma,
                     prescale_r(gamma2), prescale_r(Fr::one()), tau);
}

}  // namespace lh
