// Device half of the LogUp-GKR lookup argument (logup.cpp; tests/logup_gkr_ref.py): row compression and the leaves of
// the two fractional sum-checks with the level above them.  Streaming kernels: an Fr is two dwordx4, every entry is
// read once and every result written once.  (The multiplicities are the sort-merge join of kernels_plonk.hip.)
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstring>
#include "dev.hpp"
#include "ff_host.hpp"
#include "launch.cuh"
#include "wide.cuh"

namespace lh {

// ------------------------------------------------------------------ compress: out = sum_j beta^j col_j
// One pass: width * 32 B read and 32 B written per row; the column pointers and the powers travel in the kernel arguments
struct LogupCompress {
  const Fr* col[LOGUP_MAX];
  Fr pow[LOGUP_MAX];
  int width;
};
__global__ __launch_bounds__(256) void logup_compress_kernel(LogupCompress p, size_t n, Fr* __restrict__ out) {
  GSTRIDE(i, n) {
    Fr acc = p.col[0][i];
    for (int j = 1; j < p.width; j++) acc = add(acc, mul(p.pow[j], p.col[j][i]));
    out[i] = acc;
  }
}
void k_logup_compress(Ctx& c, const Fr* const* cols, const Fr* pows, size_t width, size_t n, Fr* out) {
  LH_REQUIRE(width >= 2 && width <= (size_t)LOGUP_MAX && n >= 1, LH_ERR_ARG, "logup_compress: bad shape");
  LogupCompress p;
  memset(&p, 0, sizeof(p));
  p.width = (int)width;
  for (size_t j = 0; j < width; j++) {
    LH_REQUIRE(cols[j] != nullptr, LH_ERR_ARG, "logup_compress: null column");
    p.col[j] = cols[j], p.pow[j] = pows[j];
  }
  ProfScope ps(c, "logup_compress", (width + 1) * 32.0 * n, (width - 1.0) * n, (double)n);
  const unsigned grid = cu_grid(c, n);
  hipLaunchKernelGGL(logup_compress_kernel, dim3(grid), dim3(256), 0, c.stream, p, n, out);
}

// ------------------------------------------------------------------ compress over mixed columns: some are uint32_t
// A u32 entry is 8 multiply-adds into the row's wide accumulator (wide.cuh), reduced ONCE per row (the u32 columns' powers
// arrive times R) - instead of a conversion and a full multiplication per entry; the Fr columns of the row are multiplied as
// above and added in.  4 B or 32 B read per column entry, 32 B written per row.  A block takes tiles of 256 ROWS rows and a
// lane the rows lane + 256 r of its tile: ROWS independent loads in flight per column, every load and every store
// lane-consecutive.  (Measured at 2^24 rows, two u32 columns: 0.21 ms this way; 0.30 ms with four CONSECUTIVE rows per lane -
// one dwordx4 per column, but 128 B of output per lane, which no store instruction coalesces; 0.23 ms with one row per lane.)
struct LogupCompressCols {
  const uint32_t* sm[LOGUP_MAX];  // the u32 columns ...
  Fr wsm[LOGUP_MAX];              // ... and their powers times R
  const Fr* fr[LOGUP_MAX];        // the Fr columns and their powers
  Fr wfr[LOGUP_MAX];
  int num_sm, num_fr;
};
// ROWS = 4: n is a multiple of 1024, no bounds to check; ROWS = 1: any n
template <int ROWS>
__global__ __launch_bounds__(256) void logup_compress_cols_kernel(LogupCompressCols p, size_t n, Fr* __restrict__ out) {
  const size_t tiles = (n + 256 * ROWS - 1) / (256 * ROWS);
  for (size_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const size_t i0 = tile * (256 * ROWS) + threadIdx.x;
    if (ROWS == 1 && i0 >= n) break;
    // one accumulator per row, indexed by constants only (an array indexed by a run-time count lives in scratch memory)
    Wide t[ROWS];
#pragma unroll
    for (int r = 0; r < ROWS; r++) t[r] = Wide::zero();
    for (int k = 0; k < p.num_sm; k++) {
      const Fr w = p.wsm[k];
#pragma unroll
      for (int r = 0; r < ROWS; r++) wide_mac(t[r], w, p.sm[k][i0 + 256 * r]);
    }
#pragma unroll
    for (int r = 0; r < ROWS; r++) {
      const size_t i = i0 + 256 * r;
      Fr acc = wide_redc(t[r]);
      for (int k = 0; k < p.num_fr; k++) acc = add(acc, mul(p.wfr[k], p.fr[k][i]));
      out[i] = acc;
    }
  }
}
void k_logup_compress_cols(Ctx& c, const void* const* cols, const uint8_t* u32, const Fr* pows, size_t width, size_t n, Fr* out) {
  LH_REQUIRE(width >= 1 && width <= (size_t)LOGUP_MAX && n >= 1, LH_ERR_ARG, "logup_compress_cols: bad shape");
  LogupCompressCols p;
  memset(&p, 0, sizeof(p));
  for (size_t j = 0; j < width; j++) {
    LH_REQUIRE(cols[j] != nullptr, LH_ERR_ARG, "logup_compress_cols: null column");
    if (u32[j]) {
      p.sm[p.num_sm] = (const uint32_t*)cols[j], p.wsm[p.num_sm++] = prescale_r(pows[j]);
    } else {
      p.fr[p.num_fr] = (const Fr*)cols[j], p.wfr[p.num_fr++] = pows[j];
    }
  }
  LH_REQUIRE(p.num_sm >= 1, LH_ERR_ARG, "logup_compress_cols: no u32 column");
  ProfScope ps(c, "logup_compress_cols", (4.0 * p.num_sm + 32.0 * p.num_fr + 32.0) * n, (0.07 * p.num_sm + 0.6 + p.num_fr) * n,
               (double)n);
  const bool four = n % 1024 == 0;
  const unsigned grid = cu_grid(c, n, four ? 1024 : 256);
  if (four) hipLaunchKernelGGL(logup_compress_cols_kernel<4>, dim3(grid), dim3(256), 0, c.stream, p, n, out);
  else hipLaunchKernelGGL(logup_compress_cols_kernel<1>, dim3(grid), dim3(256), 0, c.stream, p, n, out);
}

// ------------------------------------------------------------------ leaves (+ the level above) of a side's fractions
// Lane i < half makes the leaves i and i + half of fraction blockIdx.y - the pair Layer::up joins - and with UP their node.
//   !TABLE: q = gamma + c, p == 1 (fraction 0's lanes fill the shared table of ones); node = (q_l + q_r, q_l q_r)
//    TABLE: p = -m, q = gamma + c;                                                    node = (p_l q_r + p_r q_l, q_l q_r)
template <bool TABLE, bool UP>
__global__ __launch_bounds__(256) void logup_leaves_kernel(LogupLeaves a, size_t half, Fr gamma) {
  const unsigned k = blockIdx.y;
  const Fr* __restrict__ const col = a.c[k];
  Fr* __restrict__ const q = a.q[k];
  GSTRIDE(i, half) {
    const Fr ql = add(gamma, col[i]), qr = add(gamma, col[i + half]);
    q[i] = ql;
    q[i + half] = qr;
    if (TABLE) {
      const Fr pl = neg(from_u64<FrParams>(a.m[k][i])), pr = neg(from_u64<FrParams>(a.m[k][i + half]));
      a.p[k][i] = pl;
      a.p[k][i + half] = pr;
      if (UP) a.p_up[k][i] = add(mul(pl, qr), mul(pr, ql));
    } else {
      if (k == 0) {
        a.ones[i] = Fr::one();
        a.ones[i + half] = Fr::one();
      }
      if (UP) a.p_up[k][i] = add(ql, qr);
    }
    if (UP) a.q_up[k][i] = mul(ql, qr);
  }
}
void k_logup_leaves(Ctx& c, const LogupLeaves& a, size_t count, size_t num_vars, bool table_side, bool up, const Fr& gamma) {
  LH_REQUIRE(count >= 1 && count <= (size_t)LOGUP_MAX && num_vars >= 1 && num_vars < 32, LH_ERR_ARG, "logup_leaves: bad shape");
  for (size_t k = 0; k < count; k++)
    LH_REQUIRE(a.c[k] && a.q[k] && (table_side ? a.m[k] && a.p[k] : a.ones != nullptr) && (!up || (a.p_up[k] && a.q_up[k])),
               LH_ERR_ARG, "logup_leaves: null column");
  const size_t half = (size_t)1 << (num_vars - 1);
  const double per = table_side ? 2 * (4.0 + 32.0 + 64.0) + (up ? 64.0 : 0.0) : 2 * (32.0 + 32.0) + (up ? 64.0 : 0.0);
  ProfScope ps(c, up ? "logup_leaves_up" : "logup_leaves", per * half * count + (table_side ? 0.0 : 64.0 * half),
               ((table_side ? 2.0 : 0.0) + (up ? (table_side ? 3.0 : 1.0) : 0.0)) * half * count, (double)half * count);
  const dim3 grid(cu_grid(c, half), (unsigned)count);
  if (table_side && up) hipLaunchKernelGGL((logup_leaves_kernel<true, true>), grid, dim3(256), 0, c.stream, a, half, gamma);
  else if (table_side) hipLaunchKernelGGL((logup_leaves_kernel<true, false>), grid, dim3(256), 0, c.stream, a, half, gamma);
  else if (up) hipLaunchKernelGGL((logup_leaves_kernel<false, true>), grid, dim3(256), 0, c.stream, a, half, gamma);
  else hipLaunchKernelGGL((logup_leaves_kernel<false, false>), grid, dim3(256), 0, c.stream, a, half, gamma);
}

}  // namespace lh
