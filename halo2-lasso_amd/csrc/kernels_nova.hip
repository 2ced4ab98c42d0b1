// Device half of Nova folding (nova.cpp; tests/nova_ref.py): the keyed field sum of kernels_spartan.hip with TWO right-hand
// sides in one pass over the key's sorted entry stream - the six products A z1 .. C z2 of a fold -, the cross term with the
// count of the rows at which an input fails its own relaxed relation, the count alone (the relaxed prover's), and the
// linear combination of witnesses and error vectors.  Field sums are exact: the bytes do not depend on the order of addition.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstring>
#include "dev.hpp"
#include "ff_host.hpp"
#include "launch.cuh"
#include "reduce.cuh"
#include "spmv.cuh"

namespace lh {

// ------------------------------------------------------------------ the keyed sum, two right-hand sides
// wave_segmented_sum (spmv.cuh) over a pair of values under one key: 16 limbs travel per step, the key once
__device__ __forceinline__ void wave_segmented_sum2(uint32_t key, Fr& va, Fr& vb, bool& tail, bool& from0) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t ko = __shfl_up(key, off, 64);
    Fr oa, ob;
#pragma unroll
    for (int i = 0; i < 8; i++) oa.l[i] = __shfl_up(va.l[i], off, 64), ob.l[i] = __shfl_up(vb.l[i], off, 64);
    if (lane >= off && ko == key) va = add(va, oa), vb = add(vb, ob);
  }
  tail = lane == 63 || __shfl_down(key, 1, 64) != key;
  from0 = __shfl(key, 0, 64) == key;
}

// wave_store_or_carry (spmv.cuh) for the pair: the same three ways, one carry item of key and two sums (68 B)
__device__ __forceinline__ void wave_store_or_carry2(uint32_t key, const Fr& va, const Fr& vb, bool tail, bool from0, Fr* out_a,
                                                     Fr* out_b, uint32_t* ck, Fr* ca, Fr* cb) {
  const int lane = threadIdx.x & 63;
  if (!tail) return;
  if (from0) {
    ck[0] = key, ca[0] = va, cb[0] = vb;
    if (lane == 63) ck[1] = key, ca[1] = Fr::zero(), cb[1] = Fr::zero();
  } else if (lane == 63) {
    ck[1] = key, ca[1] = va, cb[1] = vb;
  } else if (key != SPMV_NO_KEY) {
    out_a[key] = va, out_b[key] = vb;
  }
}

// blockIdx.x: the tile, blockIdx.y: the matrix.  Per entry: key, other index and position (12 B, coalesced), the value
// through the position (32 B gather) - all once for both sides -, X1[other] and X2[other] (32 B gathers at one index), two
// products, twelve conditional additions of the wave scan.  LDS: the tile's 64 carry items of 68 B.
__global__ __launch_bounds__(256) void nova_spmv2_kernel(NovaSpmv2 p, size_t n, uint32_t mask, unsigned tiles) {
  __shared__ Fr item_a[2 * SPMV_ROWS];
  __shared__ Fr item_b[2 * SPMV_ROWS];
  __shared__ uint32_t item_k[2 * SPMV_ROWS];
  const unsigned m = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t* __restrict__ seg = p.seg[m];
  const uint32_t* __restrict__ other = p.other[m];
  const uint32_t* __restrict__ perm = p.perm[m];
  const Fr* __restrict__ val = p.val[m];
  const Fr* X1 = p.X1;  // (may be one vector)
  const Fr* X2 = p.X2;
  Fr* __restrict__ out_a = p.out1[m];
  Fr* __restrict__ out_b = p.out2[m];
  const size_t base = (size_t)blockIdx.x * SPMV_TILE;
  for (unsigned row = wave; row < (unsigned)SPMV_ROWS; row += 4) {
    const size_t k = base + (size_t)row * 64 + lane;
    uint32_t key = SPMV_NO_KEY;
    Fr va = Fr::zero(), vb = Fr::zero();
    if (k < n) {
      key = seg[k] & mask;
      const Fr v = val[perm[k] & (uint32_t)(n - 1)];
      const uint32_t o = other[k] & mask;
      va = mul(v, X1[o]), vb = mul(v, X2[o]);
    }
    bool tail, from0;
    wave_segmented_sum2(key, va, vb, tail, from0);
    wave_store_or_carry2(key, va, vb, tail, from0, out_a, out_b, item_k + 2 * row, item_a + 2 * row, item_b + 2 * row);
  }
  __syncthreads();
  if (wave == 0) {  // the 64 carry items of the tile: the same step once more, its two carries go to the fold kernel
    const uint32_t key = item_k[lane];
    Fr va = item_a[lane], vb = item_b[lane];
    bool tail, from0;
    wave_segmented_sum2(key, va, vb, tail, from0);
    const size_t at = ((size_t)m * tiles + blockIdx.x) * 2;
    wave_store_or_carry2(key, va, vb, tail, from0, out_a, out_b, p.carry_k + at, p.carry_v1 + at, p.carry_v2 + at);
  }
}

// spartan_spmv_fold_kernel for the pair: ONE wave per matrix walks the 2 * tiles carries with the running key and sums of
// the segment that is still open.  Every segment that reaches this kernel is stored here and nowhere else.
__global__ __launch_bounds__(64) void nova_spmv2_fold_kernel(NovaSpmv2 p, unsigned tiles) {
  const unsigned m = blockIdx.x, lane = threadIdx.x;
  const size_t count = (size_t)2 * tiles;
  const uint32_t* __restrict__ ck = p.carry_k + (size_t)m * count;
  const Fr* __restrict__ ca = p.carry_v1 + (size_t)m * count;
  const Fr* __restrict__ cb = p.carry_v2 + (size_t)m * count;
  Fr* __restrict__ out_a = p.out1[m];
  Fr* __restrict__ out_b = p.out2[m];
  uint32_t open_key = SPMV_NO_KEY;
  Fr open_a = Fr::zero(), open_b = Fr::zero();
  for (size_t b = 0; b < count; b += 64) {
    const size_t i = b + lane;
    const uint32_t key = i < count ? ck[i] : SPMV_NO_KEY;
    Fr va = i < count ? ca[i] : Fr::zero(), vb = i < count ? cb[i] : Fr::zero();
    bool tail, from0;
    wave_segmented_sum2(key, va, vb, tail, from0);
    const uint32_t key0 = __shfl(key, 0, 64);
    if (open_key == key0) {
      if (from0) va = add(va, open_a), vb = add(vb, open_b);
    } else if (lane == 0 && open_key != SPMV_NO_KEY) {
      out_a[open_key] = open_a, out_b[open_key] = open_b;
    }
    if (tail && lane != 63 && key != SPMV_NO_KEY) out_a[key] = va, out_b[key] = vb;
    open_key = __shfl(key, 63, 64);
#pragma unroll
    for (int j = 0; j < 8; j++) open_a.l[j] = __shfl(va.l[j], 63, 64), open_b.l[j] = __shfl(vb.l[j], 63, 64);
  }
  if (lane == 0 && open_key != SPMV_NO_KEY) out_a[open_key] = open_a, out_b[open_key] = open_b;
}

void k_nova_spmv2(Ctx& c, const NovaSpmv2& p, size_t n, size_t dim_vars) {
  LH_REQUIRE(n >= 1 && (n & (n - 1)) == 0 && n <= ((size_t)1 << 31) && dim_vars >= 1 && dim_vars <= 24, LH_ERR_ARG,
             "nova_spmv2: bad shape");
  LH_REQUIRE(p.X1 && p.X2, LH_ERR_ARG, "nova_spmv2: null column");
  for (int m = 0; m < 3; m++)
    LH_REQUIRE(p.seg[m] && p.other[m] && p.perm[m] && p.val[m] && p.out1[m] && p.out2[m], LH_ERR_ARG, "nova_spmv2: null column");
  const size_t cells = (size_t)1 << dim_vars;
  const unsigned tiles = (unsigned)((n + SPMV_TILE - 1) / SPMV_TILE);
  // per entry 12 B of key, other index and position, the value, X1[other] and X2[other] (32 B each); per cell two sums
  ProfScope ps(c, "nova_spmv2", 3.0 * (108.0 * n + 64.0 * cells), 6.0 * n, 3.0 * n);
  ArenaScope scope(c.arena);
  NovaSpmv2 a = p;
  a.carry_k = c.arena.alloc_n<uint32_t>((size_t)6 * tiles);
  a.carry_v1 = c.arena.alloc_n<Fr>((size_t)6 * tiles);
  a.carry_v2 = c.arena.alloc_n<Fr>((size_t)6 * tiles);
  // a segment without entries is zero: nothing is left to what the caller's buffers held
  for (int m = 0; m < 3; m++) {
    LH_HIP(hipMemsetAsync(a.out1[m], 0, cells * sizeof(Fr), c.stream));
    LH_HIP(hipMemsetAsync(a.out2[m], 0, cells * sizeof(Fr), c.stream));
  }
  hipLaunchKernelGGL(nova_spmv2_kernel, dim3(tiles, 3), dim3(256), 0, c.stream, a, n, (uint32_t)(cells - 1), tiles);
  hipLaunchKernelGGL(nova_spmv2_fold_kernel, dim3(3), dim3(64), 0, c.stream, a, tiles);
}

// ------------------------------------------------------------------ the cross term and the rows that fail
// a b != u c + e (e null: zero); the values are canonical, so limbs compare
__device__ __forceinline__ bool relaxed_row_fails(const Fr& a, const Fr& b, const Fr& c, const Fr& u, const Fr* e, size_t i) {
  const Fr prod = mul(a, b);
  Fr want = mul(u, c);
  if (e) want = add(want, e[i]);
  bool same = true;
#pragma unroll
  for (int j = 0; j < 8; j++) same = same && prod.l[j] == want.l[j];
  return !same;
}
// the workgroup's counts into count[0 .. K): wave shuffles, LDS across the four waves, one integer atomic per counter
template <int K>
__device__ __forceinline__ void block_count(uint32_t (&bad)[K], uint32_t* count) {
  __shared__ uint32_t lds[4][K];
#pragma unroll
  for (int k = 0; k < K; k++) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) bad[k] += __shfl_down(bad[k], off, 64);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6][k] = bad[k];
  }
  __syncthreads();
  if (threadIdx.x < K) {
    const uint32_t total = lds[0][threadIdx.x] + lds[1][threadIdx.x] + lds[2][threadIdx.x] + lds[3][threadIdx.x];
    if (total) atomicAdd(count + threadIdx.x, total);
  }
}

// T = Az1 Bz2 + Az2 Bz1 - u1 Cz2 - u2 Cz1 as four Montgomery products and three additions: wide.cuh's accumulate-then-reduce
// takes weights times 32-bit integers, not full-width products, so the plain form is the one kept (exact either way).
__global__ __launch_bounds__(256) void nova_cross_term_kernel(NovaCross p, Fr u1, Fr u2, size_t rows, uint32_t* count) {
  uint32_t bad[2] = {0, 0};
  GSTRIDE(i, rows) {
    const Fr a1 = p.mz1[0][i], b1 = p.mz1[1][i], c1 = p.mz1[2][i];
    const Fr a2 = p.mz2[0][i], b2 = p.mz2[1][i], c2 = p.mz2[2][i];
    bad[0] += relaxed_row_fails(a1, b1, c1, u1, p.e1, i);
    bad[1] += relaxed_row_fails(a2, b2, c2, u2, p.e2, i);
    p.t[i] = sub(sub(add(mul(a1, b2), mul(a2, b1)), mul(u1, c2)), mul(u2, c1));
  }
  block_count<2>(bad, count);
}
void k_nova_cross_term(Ctx& c, const NovaCross& p, const Fr& u1, const Fr& u2, size_t rows, size_t bad[2]) {
  LH_REQUIRE(rows >= 1 && p.t, LH_ERR_ARG, "nova_cross_term: bad arguments");
  for (int m = 0; m < 3; m++) LH_REQUIRE(p.mz1[m] && p.mz2[m], LH_ERR_ARG, "nova_cross_term: null column");
  ProfScope ps(c, "nova_cross_term", 32.0 * rows * (7 + (p.e1 != nullptr) + (p.e2 != nullptr)), 8.0 * rows, (double)rows);
  ArenaScope scope(c.arena);
  uint32_t* count = c.arena.alloc_n<uint32_t>(2);
  LH_HIP(hipMemsetAsync(count, 0, 2 * sizeof(uint32_t), c.stream));
  hipLaunchKernelGGL(nova_cross_term_kernel, dim3(cu_grid(c, rows)), dim3(256), 0, c.stream, p, u1, u2, rows, count);
  uint32_t host[2] = {0, 0};
  c.d2h(host, count, sizeof(host));
  bad[0] = host[0], bad[1] = host[1];
}

__global__ __launch_bounds__(256) void nova_unsatisfied_kernel(const Fr* __restrict__ az, const Fr* __restrict__ bz,
                                                              const Fr* __restrict__ cz, Fr u, const Fr* __restrict__ e, size_t rows,
                                                              uint32_t* count) {
  uint32_t bad[1] = {0};
  GSTRIDE(i, rows) bad[0] += relaxed_row_fails(az[i], bz[i], cz[i], u, e, i);
  block_count<1>(bad, count);
}
size_t k_nova_unsatisfied(Ctx& c, const Fr* az, const Fr* bz, const Fr* cz, const Fr& u, const Fr* e, size_t rows) {
  LH_REQUIRE(az && bz && cz && rows >= 1, LH_ERR_ARG, "nova_unsatisfied: bad arguments");
  ProfScope ps(c, "nova_unsatisfied", 32.0 * rows * (3 + (e != nullptr)), 2.0 * rows, (double)rows);
  ArenaScope scope(c.arena);
  uint32_t* count = c.arena.alloc_n<uint32_t>(1);
  LH_HIP(hipMemsetAsync(count, 0, sizeof(uint32_t), c.stream));
  hipLaunchKernelGGL(nova_unsatisfied_kernel, dim3(cu_grid(c, rows)), dim3(256), 0, c.stream, az, bz, cz, u, e, rows, count);
  uint32_t host = 0;
  c.d2h(&host, count, sizeof(host));
  return host;
}

// ------------------------------------------------------------------ the linear combination
// w_out[i] = w1[i] + r w2[i] for i < half, then e_out[j] = e1[j] + r t[j] + r^2 e2[j] for j < rows (e1, e2 null: zero), two
// grid-stride loops of one launch.  An element is read before it is written and by its own lane alone: the outputs may be
// the first (or second) input.
__global__ __launch_bounds__(256) void nova_fold_kernel(const Fr* w1, const Fr* w2, Fr* w_out, const Fr* e1, const Fr* t, const Fr* e2,
                                                       Fr* e_out, Fr r, Fr r2, size_t half, size_t rows) {
  GSTRIDE(i, half) w_out[i] = add(w1[i], mul(r, w2[i]));
  GSTRIDE(j, rows) {
    Fr v = mul(r, t[j]);
    if (e1) v = add(v, e1[j]);
    if (e2) v = add(v, mul(r2, e2[j]));
    e_out[j] = v;
  }
}
void k_nova_fold(Ctx& c, const Fr* w1, const Fr* w2, Fr* w_out, const Fr* e1, const Fr* t, const Fr* e2, Fr* e_out, const Fr& r,
                 const Fr& r2, size_t half, size_t rows) {
  LH_REQUIRE(w1 && w2 && w_out && t && e_out && half >= 1 && rows >= 1, LH_ERR_ARG, "nova_fold: bad arguments");
  const size_t items = half + rows;
  ProfScope ps(c, "nova_fold", 96.0 * half + 32.0 * rows * (2 + (e1 != nullptr) + (e2 != nullptr)),
               (double)half + (double)rows * (1 + (e2 != nullptr)), (double)items);
  hipLaunchKernelGGL(nova_fold_kernel, dim3(cu_grid(c, rows)), dim3(256), 0, c.stream, w1, w2, w_out, e1, t, e2, e_out, r, r2, half, rows);
}

}  // namespace lh
