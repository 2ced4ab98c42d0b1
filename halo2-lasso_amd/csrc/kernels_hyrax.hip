// Row commitments of Hyrax (reference pcs/multilinear/hyrax.rs:169-221): out[r] = sum_c s[r row_len + c] g[c]
// for EVERY row of EVERY column of a batch against the same generators, in one pass and without a host wait in between.
// The generators come as their window table (k_msm_window_table: entry w row_len + i = 2^(8 w) g[i]), so every
// (window, column) term of a row is ONE mixed addition into ONE bucket set per row and no doubling is ever made.
//   rows_msm       one workgroup per (row, segment of columns): the digits of its scalars (signed for Fr: buckets 1..128,
//                  unsigned for u32: buckets 1..255) are counted and grouped per bucket by a counting sort in LDS, every
//                  thread adds the terms of the bucket(s) it owns (complete XYZZ additions: equal bases, opposite bases and
//                  identities are ordinary operands), the workgroup reduces sum_b b B_b (a suffix scan and a tree sum over
//                  LDS) and thread 0 stores one XYZZ point.  No global sort, no global buckets, no atomics on points.
//   rows_sum       the segments' points of a row added up (rows longer than one segment only)
//   rows_normalize every row of the batch affine behind batched inversions; the identity comes out as (0, 0)
// Rows that lie wholly beyond a column's n entries get no workgroup: their points are the zero bytes of a memset.
#include <hip/hip_runtime.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "dev.hpp"

namespace lh {

constexpr uint32_t RM_THREADS = 128;
constexpr uint32_t RM_CBITS = 8;            // digits are the scalar's bytes
constexpr uint32_t RM_W_FR = 32;            // ceil(255 / 8): byte 31 of a canonical scalar is <= 0x30, it absorbs the last carry
constexpr uint32_t RM_MAX_TERMS = 8192;     // (column, window) terms of one workgroup: 13 bits of a 16-bit entry + the sign
constexpr uint32_t RM_SEG_LOG_FR = 8;       // columns per workgroup: 256 x 32 windows
constexpr uint32_t RM_SEG_LOG_U32 = 11;     // 2048 x (<= 4) windows
constexpr uint32_t RM_MAX_COLS = 48;        // columns of one launch (the descriptors travel as kernel arguments)
constexpr size_t RM_MAX_PARTIALS = (size_t)1 << 19;  // segment points of one launch (64 MiB), unless one column needs more
static_assert((RM_W_FR << RM_SEG_LOG_FR) <= RM_MAX_TERMS && (4u << RM_SEG_LOG_U32) <= RM_MAX_TERMS, "term ids fit 13 bits");

struct RowsColDev {
  const void* scalars;
  uint64_t n;            // entries present (the rest of the last live row is zero)
  uint64_t out_base;     // where the workgroups' points go: + row * segs + seg
  uint64_t sum_base;     // where the row sums go: + row (segs > 1)
  uint32_t first_block;  // of this column in the launch
  uint32_t first_row;    // of this column among the rows rows_sum adds up in this launch
  uint32_t live_rows;    // ceil(n / row_len)
  uint32_t segs;         // workgroups per row
  uint32_t seg_log;
  uint32_t W;            // windows of this column
  uint32_t is_u32;
  uint32_t pad;
};
struct RowsLaunch {
  RowsColDev col[RM_MAX_COLS];
  uint32_t num_cols;
  uint32_t sum_rows;  // rows of this launch that have more than one segment
  uint32_t sum_T;     // threads per such row (a power of two <= 64)
  uint32_t pad;
  uint64_t row_len;
};
static_assert(sizeof(RowsLaunch) <= 4096 - 64, "kernel arguments stay below 4 KB");

// the W digits of one scalar (limbs least significant first), f(window, digit, negative); digit 0 is not reported
template <class F>
__device__ __forceinline__ void rows_digits(Fr s, uint32_t W, bool is_signed, F f) {
  uint32_t carry = 0;
#pragma unroll 1
  for (uint32_t k = 0; 4 * k < W; k++) {  // rolled: the limbs rotate through s.l[0] so that indexing stays static
    const uint32_t limb = s.l[0];
#pragma unroll
    for (int q = 0; q < 7; q++) s.l[q] = s.l[q + 1];
#pragma unroll
    for (uint32_t b = 0; b < 4; b++) {
      const uint32_t w = 4 * k + b;
      if (w >= W) break;
      uint32_t d = ((limb >> (8 * b)) & 0xffu) + carry, neg = 0;
      if (is_signed) {
        carry = d > 128u ? 1u : 0u;
        if (carry) d = 256u - d, neg = 1;
      }
      if (d) f(w, d, neg);
    }
  }
}

__device__ __forceinline__ Fr rows_load(const RowsColDev& cd, uint64_t idx) {
  if (!cd.is_u32) return from_mont(((const Fr*)cd.scalars)[idx]);
  Fr s = Fr::zero();
  s.l[0] = ((const uint32_t*)cd.scalars)[idx];
  return s;
}

__global__ __launch_bounds__(RM_THREADS) void rows_msm_kernel(RowsLaunch L, const G1Affine* __restrict__ table,
                                                              G1Xyzz* __restrict__ pts) {
  __shared__ uint32_t cnt[258], start[258], scan[RM_THREADS];
  __shared__ __align__(16) unsigned char pool[RM_THREADS * sizeof(G1Xyzz)];  // the sorted terms, then the workgroup's points
  static_assert(sizeof(pool) >= RM_MAX_TERMS * sizeof(uint16_t), "pool holds the sorted terms");
  uint16_t* sorted = (uint16_t*)pool;
  G1Xyzz* lp = (G1Xyzz*)pool;
  const uint32_t t = threadIdx.x;

  uint32_t k = 0;
  while (k + 1 < L.num_cols && blockIdx.x >= L.col[k + 1].first_block) k++;
  const RowsColDev& cd = L.col[k];
  const uint32_t local = blockIdx.x - cd.first_block;
  const uint32_t row = local / cd.segs, seg = local - row * cd.segs;
  const uint64_t col0 = (uint64_t)seg << cd.seg_log, row_base = (uint64_t)row * L.row_len;
  uint64_t live = std::min<uint64_t>((uint64_t)1 << cd.seg_log, L.row_len - col0);
  live = row_base + col0 >= cd.n ? 0 : std::min<uint64_t>(live, cd.n - row_base - col0);
  const bool is_signed = !cd.is_u32;
  const uint32_t K = cd.is_u32 ? 2u : 1u, NB = cd.is_u32 ? 255u : 128u;  // buckets per thread, buckets

  for (uint32_t i = t; i < 258; i += RM_THREADS) cnt[i] = 0;
  __syncthreads();
  for (uint32_t j = t; j < live; j += RM_THREADS)
    rows_digits(rows_load(cd, row_base + col0 + j), cd.W, is_signed, [&](uint32_t, uint32_t d, uint32_t) { atomicAdd(&cnt[d], 1u); });
  __syncthreads();
  {  // exclusive prefix sums over the 256 counters, two per thread
    const uint32_t c0 = cnt[2 * t], c1 = cnt[2 * t + 1];
    scan[t] = c0 + c1;
    __syncthreads();
    for (uint32_t off = 1; off < RM_THREADS; off <<= 1) {
      const uint32_t v = t >= off ? scan[t - off] : 0;
      __syncthreads();
      scan[t] += v;
      __syncthreads();
    }
    const uint32_t excl = scan[t] - (c0 + c1);
    start[2 * t] = excl, start[2 * t + 1] = excl + c0;
    cnt[2 * t] = excl, cnt[2 * t + 1] = excl + c0;  // from here on: the next free place of the bucket
  }
  __syncthreads();
  for (uint32_t j = t; j < live; j += RM_THREADS)
    rows_digits(rows_load(cd, row_base + col0 + j), cd.W, is_signed, [&](uint32_t w, uint32_t d, uint32_t neg) {
      const uint32_t pos = atomicAdd(&cnt[d], 1u);
      sorted[pos] = (uint16_t)(((w << cd.seg_log) + j) | (neg << 15));
    });
  __syncthreads();

  // thread t owns the buckets K t + 1 .. K t + K: P = their sum, Lw = sum_i i B_{K t + i}
  G1Xyzz P = G1Xyzz::identity(), Lw = G1Xyzz::identity();
  for (uint32_t i = 1; i <= K; i++) {
    const uint32_t b = K * t + i;
    if (b > NB) break;
    G1Xyzz acc = G1Xyzz::identity();
    const uint32_t end = cnt[b];
    for (uint32_t p = start[b]; p < end; p++) {
      const uint32_t e = sorted[p], id = e & 0x1fffu;
      const uint64_t w = id >> cd.seg_log, j = id & ((1u << cd.seg_log) - 1u);
      acc = add_mixed(acc, table[w * L.row_len + col0 + j], (e >> 15) != 0);
    }
    if (i == 1) {
      P = acc, Lw = acc;
    } else {
      P = add(P, acc);
      Lw = add(P, acc);  // B_1 + 2 B_2
    }
  }
  __syncthreads();  // the sorted terms are read: the pool becomes the points

  // sum_b b B_b = K sum_{t >= 1} S_t + sum_t Lw_t with S_t = sum_{u >= t} P_u
  lp[t] = P;
  __syncthreads();
  for (uint32_t off = 1; off < RM_THREADS; off <<= 1) {
    const bool has = t + off < RM_THREADS;
    G1Xyzz o;
    if (has) o = lp[t + off];
    __syncthreads();
    if (has) {
      P = add(P, o);
      lp[t] = P;
    }
    __syncthreads();
  }
  G1Xyzz V = Lw;
  if (t >= 1) V = add(V, K == 2 ? dbl(P) : P);
  lp[t] = V;
  __syncthreads();
  for (uint32_t off = RM_THREADS / 2; off > 0; off >>= 1) {
    if (t < off) {
      V = add(V, lp[t + off]);
      lp[t] = V;
    }
    __syncthreads();
  }
  if (t == 0) pts[cd.out_base + local] = V;
}

// sums[row] = the sum of the row's `segs` points: sum_T threads per row, a tree over LDS
__global__ __launch_bounds__(64) void rows_sum_kernel(RowsLaunch L, G1Xyzz* __restrict__ pts) {
  __shared__ G1Xyzz lp[64];
  const uint32_t T = L.sum_T, per_block = 64 / T;
  const uint32_t g = blockIdx.x * per_block + threadIdx.x / T, lane = threadIdx.x % T;
  const bool valid = g < L.sum_rows;
  G1Xyzz acc = G1Xyzz::identity();
  uint32_t k = 0, row = 0;
  if (valid) {
    while (k + 1 < L.num_cols && g >= L.col[k + 1].first_row) k++;
    row = g - L.col[k].first_row;
    const RowsColDev& cd = L.col[k];
    for (uint32_t s = lane; s < cd.segs; s += T) acc = add(acc, pts[cd.out_base + (uint64_t)row * cd.segs + s]);
  }
  lp[threadIdx.x] = acc;
  __syncthreads();
  for (uint32_t off = T / 2; off > 0; off >>= 1) {
    if (valid && lane < off) {
      acc = add(acc, lp[threadIdx.x + off]);
      lp[threadIdx.x] = acc;
    }
    __syncthreads();
  }
  if (valid && lane == 0) pts[L.col[k].sum_base + row] = acc;
}

// (the normalisation of kernels_ipa.hip's base fold: RN_BATCH points behind one inversion, an identity takes the place of
// a one in the running product)
constexpr int RN_BATCH = 8;
__global__ __launch_bounds__(128) void rows_normalize_kernel(const G1Xyzz* __restrict__ sums, size_t n, G1Affine* __restrict__ out) {
  const size_t groups = (n + RN_BATCH - 1) / RN_BATCH;
  for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (size_t)gridDim.x * blockDim.x) {
    const size_t i0 = g * RN_BATCH;
    Fq pre[RN_BATCH];
    Fq run = Fq::one();
#pragma unroll
    for (int k = 0; k < RN_BATCH; k++) {
      pre[k] = run;
      if (i0 + k < n) {
        const Fq zz = sums[i0 + k].zz;
        if (!zz.is_zero()) run = mul(run, mul(zz, sums[i0 + k].zzz));
      }
    }
    Fq iv = inv(run);  // (a product of nonzero elements)
#pragma unroll
    for (int k = RN_BATCH - 1; k >= 0; k--) {
      if (i0 + k >= n) continue;
      const G1Xyzz p = sums[i0 + k];
      G1Affine r;
      if (p.is_identity()) {
        r.x = Fq::zero(), r.y = Fq::zero();
      } else {
        const Fq di = mul(iv, pre[k]);  // 1 / (ZZ ZZZ)
        iv = mul(iv, mul(p.zz, p.zzz));
        r.x = mul(p.x, mul(di, p.zzz));
        r.y = mul(p.y, mul(di, p.zz));
      }
      out[i0 + k] = r;
    }
  }
}

uint32_t g1_rows_msm_windows(bool u32, uint32_t bits) { return u32 ? (bits + RM_CBITS - 1) / RM_CBITS : RM_W_FR; }
size_t g1_rows_msm_segment(bool u32) { return (size_t)1 << (u32 ? RM_SEG_LOG_U32 : RM_SEG_LOG_FR); }

void k_g1_rows_msm_batch(Ctx& c, const RowsMsmCol* cols, size_t num_cols, size_t rows_per_col, size_t row_len,
                         const G1Affine* bases, const G1Affine* win_table, uint32_t cbits, uint32_t W, G1Affine* out_host) {
  const size_t total_rows = num_cols * rows_per_col;
  if (!total_rows) return;
  LH_REQUIRE(row_len >= 1 && row_len <= ((size_t)1 << 32), LH_ERR_ARG, "rows msm: row_len must be in 1..2^32");
  LH_REQUIRE(total_rows < ((size_t)1 << 31), LH_ERR_ARG, "rows msm: too many rows");
  uint32_t need_W = 0;
  for (size_t i = 0; i < num_cols; i++) {
    const RowsMsmCol& in = cols[i];
    LH_REQUIRE(!in.u32 || (in.bits >= 1 && in.bits <= 32), LH_ERR_ARG, "rows msm: bits of a u32 column must be in 1..32");
    LH_REQUIRE(in.n <= rows_per_col * row_len, LH_ERR_ARG, "rows msm: a column is longer than its rows");
    LH_REQUIRE(in.n == 0 || in.scalars != nullptr, LH_ERR_ARG, "rows msm: null column");
    if (in.n) need_W = std::max(need_W, g1_rows_msm_windows(in.u32, in.bits));
  }
  ArenaScope scope(c.arena);
  if (!win_table && need_W) {  // a temporary table of the windows this batch needs
    LH_REQUIRE(bases != nullptr, LH_ERR_ARG, "rows msm: null bases");
    G1Affine* tmp = c.arena.alloc_n<G1Affine>(row_len * need_W);
    k_msm_window_table(c, bases, row_len, RM_CBITS, need_W, tmp);
    win_table = tmp, cbits = RM_CBITS, W = need_W;
  }
  LH_REQUIRE(!need_W || (cbits == RM_CBITS && W >= need_W), LH_ERR_ARG, "rows msm: the window table must have 8-bit windows, 32 for Fr columns");
  ProfScope ps(c, "rows_msm", 0, 0, (double)total_rows);

  // the launches: up to RM_MAX_COLS columns and RM_MAX_PARTIALS segment points each
  std::vector<RowsLaunch> launches;
  std::vector<size_t> blocks_of;
  size_t max_partials = 0;
  {
    RowsLaunch L;
    memset(&L, 0, sizeof L);
    L.row_len = row_len, L.sum_T = 1;
    size_t blocks = 0, partials = 0;
    auto flush = [&]() {
      if (!L.num_cols) return;
      launches.push_back(L), blocks_of.push_back(blocks);
      max_partials = std::max(max_partials, partials);
      memset(&L, 0, sizeof L);
      L.row_len = row_len, L.sum_T = 1;
      blocks = partials = 0;
    };
    for (size_t i = 0; i < num_cols; i++) {
      const RowsMsmCol& in = cols[i];
      if (!in.n) continue;
      const uint32_t seg_log = in.u32 ? RM_SEG_LOG_U32 : RM_SEG_LOG_FR;
      const size_t live_rows = (in.n + row_len - 1) / row_len, segs = (row_len + ((size_t)1 << seg_log) - 1) >> seg_log;
      const size_t nb = live_rows * segs, np = segs > 1 ? nb : 0;
      LH_REQUIRE(nb < ((size_t)1 << 31), LH_ERR_ARG, "rows msm: a column has too many segments");
      if (L.num_cols == RM_MAX_COLS || (L.num_cols && (partials + np > RM_MAX_PARTIALS || blocks + nb >= ((size_t)1 << 31)))) flush();
      RowsColDev& cd = L.col[L.num_cols++];
      cd.scalars = in.scalars, cd.n = in.n;
      cd.sum_base = i * rows_per_col;
      cd.out_base = segs > 1 ? total_rows + partials : cd.sum_base;
      cd.first_block = (uint32_t)blocks, cd.first_row = L.sum_rows;
      cd.live_rows = (uint32_t)live_rows, cd.segs = (uint32_t)segs, cd.seg_log = seg_log;
      cd.W = g1_rows_msm_windows(in.u32, in.bits), cd.is_u32 = in.u32 ? 1 : 0;
      blocks += nb, partials += np;
      if (segs > 1) {
        L.sum_rows += (uint32_t)live_rows;
        while (L.sum_T < 64 && L.sum_T < segs) L.sum_T <<= 1;
      }
    }
    flush();
  }
  G1Xyzz* pts = c.arena.alloc_n<G1Xyzz>(total_rows + max_partials);
  G1Affine* d_out = c.arena.alloc_n<G1Affine>(total_rows);
  LH_HIP(hipMemsetAsync(pts, 0, total_rows * sizeof(G1Xyzz), c.stream));  // rows nobody computes are identities
  for (size_t l = 0; l < launches.size(); l++) {
    const RowsLaunch& L = launches[l];
    // (the first_row of a column with one segment equals its successor's: rows_sum's search passes over it)
    hipLaunchKernelGGL(rows_msm_kernel, dim3((unsigned)blocks_of[l]), dim3(RM_THREADS), 0, c.stream, L, win_table, pts);
    if (L.sum_rows) {
      const uint32_t per_block = 64 / L.sum_T;
      hipLaunchKernelGGL(rows_sum_kernel, dim3((L.sum_rows + per_block - 1) / per_block), dim3(64), 0, c.stream, L, pts);
    }
  }
  const size_t groups = (total_rows + RN_BATCH - 1) / RN_BATCH;
  hipLaunchKernelGGL(rows_normalize_kernel, dim3((unsigned)std::min<size_t>((groups + 127) / 128, 1 << 16)), dim3(128), 0, c.stream,
                     (const G1Xyzz*)pts, total_rows, d_out);
  LH_HIP(hipGetLastError());
  c.d2h(out_host, d_out, total_rows * sizeof(G1Affine));
}

void k_g1_rows_msm(Ctx& c, const void* scalars, bool u32, uint32_t bits, size_t n, size_t row_len, const G1Affine* bases,
                   const G1Affine* win_table, uint32_t cbits, uint32_t W, G1Affine* out_host) {
  LH_REQUIRE(row_len >= 1, LH_ERR_ARG, "rows msm: row_len must be at least 1");
  const RowsMsmCol col{scalars, u32, bits, n};
  k_g1_rows_msm_batch(c, &col, 1, (n + row_len - 1) / row_len, row_len, bases, win_table, cbits, W, out_host);
}

}  // namespace lh
