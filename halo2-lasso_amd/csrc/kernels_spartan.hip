// Device half of Spartan (spartan.cpp; tests/spartan_ref.py): the keyed field sum
//   out[s] = sum_{k: seg[k] = s} val[k] X[other[k]]
// that is both products of the argument - M z by rows (segments = rows, other = col, X = z) and the matrix bound at r_x by
// columns (segments = columns, other = row, X = eq(r_x, .)) - for the three matrices in one launch set, and the count of
// unsatisfied rows.  There is no 256-bit atomic: the sums are formed over the key-SORTED entry stream the R1CS key holds (no
// sort at prove time) by a segmented reduction, entry-parallel, so the cost follows the number of entries and not the longest
// segment.  Field sums are exact: the order of addition is free and the bytes do not depend on it.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstring>
#include "dev.hpp"
#include "ff_host.hpp"
#include "launch.cuh"
#include "reduce.cuh"
#include "spmv.cuh"

namespace lh {

// blockIdx.x: the tile, blockIdx.y: the matrix.  Per entry: the sorted key and the other index (4 B each, coalesced), the
// position of its value (4 B), the value (32 B gather: the entries are in the caller's order) and X[other] (32 B gather),
// one product, six conditional additions of the wave scan.  LDS: the tile's 64 carry items.
__global__ __launch_bounds__(256) void spartan_spmv_kernel(SpartanSpmv p, size_t n, uint32_t mask, unsigned tiles) {
  __shared__ Fr item_v[2 * SPMV_ROWS];
  __shared__ uint32_t item_k[2 * SPMV_ROWS];
  const unsigned m = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t* __restrict__ seg = p.seg[m];
  const uint32_t* __restrict__ other = p.other[m];
  const uint32_t* __restrict__ perm = p.perm[m];
  const Fr* __restrict__ val = p.val[m];
  const Fr* __restrict__ X = p.X;
  Fr* __restrict__ out = p.out[m];
  const size_t base = (size_t)blockIdx.x * SPMV_TILE;
  for (unsigned row = wave; row < (unsigned)SPMV_ROWS; row += 4) {
    const size_t k = base + (size_t)row * 64 + lane;
    uint32_t key = SPMV_NO_KEY;
    Fr v = Fr::zero();
    if (k < n) {
      key = seg[k] & mask;
      v = mul(val[perm[k] & (uint32_t)(n - 1)], X[other[k] & mask]);
    }
    bool tail, from0;
    v = wave_segmented_sum(key, v, tail, from0);
    wave_store_or_carry(key, v, tail, from0, out, item_k + 2 * row, item_v + 2 * row);
  }
  __syncthreads();
  if (wave == 0) {  // the 64 carry items of the tile: the same step once more, its two carries go to the fold kernel
    const uint32_t key = item_k[lane];
    bool tail, from0;
    const Fr v = wave_segmented_sum(key, item_v[lane], tail, from0);
    const size_t at = ((size_t)m * tiles + blockIdx.x) * 2;
    wave_store_or_carry(key, v, tail, from0, out, p.carry_k + at, p.carry_v + at);
  }
}

// The tiles' carries, 2 * tiles sorted items per matrix: ONE wave per matrix walks them 64 at a time with the running
// (key, sum) of the segment that is still open - a segment may span every tile.  Every segment that reaches this kernel is
// stored here and nowhere else.
__global__ __launch_bounds__(64) void spartan_spmv_fold_kernel(SpartanSpmv p, unsigned tiles) {
  const unsigned m = blockIdx.x, lane = threadIdx.x;
  const size_t count = (size_t)2 * tiles;
  const uint32_t* __restrict__ ck = p.carry_k + (size_t)m * count;
  const Fr* __restrict__ cv = p.carry_v + (size_t)m * count;
  Fr* __restrict__ out = p.out[m];
  uint32_t open_key = SPMV_NO_KEY;
  Fr open_sum = Fr::zero();
  for (size_t b = 0; b < count; b += 64) {
    const size_t i = b + lane;
    const uint32_t key = i < count ? ck[i] : SPMV_NO_KEY;
    bool tail, from0;
    Fr v = wave_segmented_sum(key, i < count ? cv[i] : Fr::zero(), tail, from0);
    const uint32_t key0 = __shfl(key, 0, 64);
    if (open_key == key0) {
      if (from0) v = add(v, open_sum);
    } else if (lane == 0 && open_key != SPMV_NO_KEY) {
      out[open_key] = open_sum;
    }
    if (tail && lane != 63 && key != SPMV_NO_KEY) out[key] = v;
    open_key = __shfl(key, 63, 64);
#pragma unroll
    for (int j = 0; j < 8; j++) open_sum.l[j] = __shfl(v.l[j], 63, 64);
  }
  if (lane == 0 && open_key != SPMV_NO_KEY) out[open_key] = open_sum;
}

void k_spartan_spmv(Ctx& c, const SpartanSpmv& p, size_t n, size_t dim_vars) {
  LH_REQUIRE(n >= 1 && (n & (n - 1)) == 0 && n <= ((size_t)1 << 31) && dim_vars >= 1 && dim_vars <= 24, LH_ERR_ARG,
             "spartan_spmv: bad shape");
  LH_REQUIRE(p.X, LH_ERR_ARG, "spartan_spmv: null column");
  for (int m = 0; m < 3; m++)
    LH_REQUIRE(p.seg[m] && p.other[m] && p.perm[m] && p.val[m] && p.out[m], LH_ERR_ARG, "spartan_spmv: null column");
  const size_t cells = (size_t)1 << dim_vars;
  const unsigned tiles = (unsigned)((n + SPMV_TILE - 1) / SPMV_TILE);
  // per entry 12 B of key, other index and position, the value and X[other] (32 B each); per cell the sum (32 B)
  ProfScope ps(c, "spartan_spmv", 3.0 * (76.0 * n + 32.0 * cells), 3.0 * n, 3.0 * n);
  ArenaScope scope(c.arena);
  SpartanSpmv a = p;
  a.carry_k = c.arena.alloc_n<uint32_t>((size_t)6 * tiles);
  a.carry_v = c.arena.alloc_n<Fr>((size_t)6 * tiles);
  // a segment without entries is zero: nothing is left to what the caller's buffers held
  for (int m = 0; m < 3; m++) LH_HIP(hipMemsetAsync(a.out[m], 0, cells * sizeof(Fr), c.stream));
  hipLaunchKernelGGL(spartan_spmv_kernel, dim3(tiles, 3), dim3(256), 0, c.stream, a, n, (uint32_t)(cells - 1), tiles);
  hipLaunchKernelGGL(spartan_spmv_fold_kernel, dim3(3), dim3(64), 0, c.stream, a, tiles);
}

// ------------------------------------------------------------------ the rows with Az Bz != Cz
__global__ __launch_bounds__(256) void spartan_unsatisfied_kernel(const Fr* __restrict__ az, const Fr* __restrict__ bz,
                                                                 const Fr* __restrict__ cz, size_t rows, uint32_t* count) {
  __shared__ uint32_t lds[4];
  uint32_t bad = 0;
  GSTRIDE(i, rows) {
    const Fr prod = mul(az[i], bz[i]), want = cz[i];
    bool same = true;
#pragma unroll
    for (int j = 0; j < 8; j++) same = same && prod.l[j] == want.l[j];
    bad += !same;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) bad += __shfl_down(bad, off, 64);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = bad;
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t total = lds[0] + lds[1] + lds[2] + lds[3];
    if (total) atomicAdd(count, total);
  }
}
size_t k_spartan_unsatisfied(Ctx& c, const Fr* az, const Fr* bz, const Fr* cz, size_t rows) {
  LH_REQUIRE(az && bz && cz && rows >= 1, LH_ERR_ARG, "spartan_unsatisfied: bad arguments");
  ProfScope ps(c, "spartan_unsatisfied", 96.0 * rows, (double)rows, (double)rows);
  ArenaScope scope(c.arena);
  uint32_t* count = c.arena.alloc_n<uint32_t>(1);
  LH_HIP(hipMemsetAsync(count, 0, sizeof(uint32_t), c.stream));
  hipLaunchKernelGGL(spartan_unsatisfied_kernel, dim3(cu_grid(c, rows)), dim3(256), 0, c.stream, az, bz, cz, rows, count);
  uint32_t host = 0;
  c.d2h(&host, count, sizeof(host));
  return host;
}

}  // namespace lh
