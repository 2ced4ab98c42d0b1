// The Reed-Solomon encoder of the Ligero PCS (tests/ligero_ref.py): number-theoretic transforms over Fr.
// A row holds its message m in its first K = 2^row_vars entries; the codeword's coset i (entries i K .. i K + K - 1,
// 0 < i < 2^b) is f(w_N^i w_K^j), f the polynomial of degree < K with f(w_K^j) = m[j], N = K 2^b.  So per row: one inverse
// transform of size K, and per parity coset a scaling of coefficient t by w_N^(i t) and one forward transform of size K.
//
// Everything is built from ONE workgroup-level step: a tile of T = C L elements (C vectors of length L, T <= 2^11) sits in
// the LDS, and the C transforms of size L run over it as log2(L) butterfly stages of T / 2 butterflies each.
//   storage     limb-interleaved: limb w of element e is the dword at w * TP + slot(e), slot(e) = e + (e >> 6),
//               TP = T + (T >> 6).  A stage's lane p works on elements (p / h) 2 h + p % h and that plus h: for h >= 32 the
//               32 lanes of a half-wave (the conflict group of the 4-byte LDS instructions, banks modulo 32) touch 32
//               consecutive dwords; for h < 32 they touch two or more runs of h, 2-way on the reads of those five stages.
//               A row-major Fr array would put lane l's limb at 8 l dwords: 8-way at every stage.  The pad (one dword per
//               64 elements) is for the load, which places element j at its bit-reversed index so that the stages run in
//               natural order: the 32 lanes of a half-wave then write at a stride of L / 32 elements, which without the pad
//               is one bank for L = 2^10 and 2^11 (32-way); with it the banks are (m + c) mod 32 or pairs of lanes
//               (2-way, which a 4-byte store does not pay for).
//   twiddles    w_(2h)^k = tw[k N / (2 h)] from the param's table of w_N^t in device memory (the inverse reads tw[N - x]);
//               k = 0 skips the product, so the first stage has none.
// Three shapes use it:
//   rs_rows     rows of K <= 2^11: C = T / K whole rows per workgroup (so K = 1 .. 64 packs 16 .. 1024 rows, not one
//               workgroup each), two tiles in the LDS: the coefficients stay in the first, each coset is scaled into the
//               second, transformed and stored.  The coefficients never leave the CU.  T = 2^8, 2^10 or 2^11.
//   rs_pass     rows of 2^12 <= K <= 2^22, four steps over K = K1 K2 (K1 = 2^floor(k/2)), index t = t1 + K1 t2 in,
//               s = s1 K2 + s2 out.  Inverse: column transforms (size K1, stride K2, C = 2^11 / K1 adjacent columns per tile,
//               so a lane group reads 32 C contiguous bytes per tile row) times w_K^-(t1 s2), written to the row's LAST coset;
//               then row transforms (size K2, contiguous) in place there: coefficient t1 + K1 t2 rests at t1 K2 + t2.
//               Forward, per coset: row transforms of the coefficients scaled by w_N^(i t) going in and by w_K^(t1 s2)
//               coming out, into the coset's own slot; then column transforms in place there, which leave natural order.
//               The last coset is computed last, in place over the coefficients.  All other cosets share two launches.
// Every global access is a whole 32-byte element per lane.  Field arithmetic is exact: the bytes are the specification's.
#include <hip/hip_runtime.h>
#include "brakedown.hpp"
#include "launch.cuh"

namespace lh {

constexpr int RS_MAX_LOG_TILE = 11;
constexpr int RS_MAX_THREADS = 512;

__device__ __forceinline__ uint32_t rs_slot(uint32_t e) { return e + (e >> 6); }
__device__ __forceinline__ Fr rs_ld(const uint32_t* buf, uint32_t tp, uint32_t e) {
  Fr v;
  const uint32_t s = rs_slot(e);
#pragma unroll
  for (int w = 0; w < 8; w++) v.l[w] = buf[w * tp + s];
  return v;
}
__device__ __forceinline__ void rs_st(uint32_t* buf, uint32_t tp, uint32_t e, const Fr& v) {
  const uint32_t s = rs_slot(e);
#pragma unroll
  for (int w = 0; w < 8; w++) buf[w * tp + s] = v.l[w];
}
__device__ __forceinline__ uint32_t rs_rev(uint32_t j, uint32_t log_l) { return log_l ? __brev(j) >> (32 - log_l) : 0; }

// the transforms of size 2^log_l over a tile of 2^log_t elements whose vectors were placed bit-reversed; natural order out
__device__ __forceinline__ void rs_tile_ntt(uint32_t* buf, uint32_t tp, uint32_t log_t, uint32_t log_l,
                                            const Fr* __restrict__ tw, uint32_t log_n, bool inverse) {
  const uint32_t half = (1u << log_t) >> 1, n_mask = (1u << log_n) - 1;
  for (uint32_t s = 0; s < log_l; s++) {
    __syncthreads();
    const uint32_t h = 1u << s;
    for (uint32_t p = threadIdx.x; p < half; p += blockDim.x) {
      const uint32_t k = p & (h - 1), i0 = ((p >> s) << (s + 1)) | k, i1 = i0 + h;
      uint32_t ti = k << (log_n - s - 1);
      if (inverse) ti = (0u - ti) & n_mask;
      const Fr u = rs_ld(buf, tp, i0);
      Fr v = rs_ld(buf, tp, i1);
      if (ti) v = mul(v, tw[ti]);
      rs_st(buf, tp, i0, add(u, v));
      rs_st(buf, tp, i1, sub(u, v));
    }
  }
  __syncthreads();
}

// ------------------------------------------------------------------ rows that fit: K <= 2^11, whole rows per workgroup
template <int LOG_T>
__global__ void __launch_bounds__(RS_MAX_THREADS)
    bd_rs_rows_kernel(Fr* __restrict__ rows, size_t cw, size_t num_rows, uint32_t log_l, uint32_t log_b,
                      const Fr* __restrict__ tw, Fr k_inv) {
  constexpr uint32_t T = 1u << LOG_T, TP = T + (T >> 6);
  __shared__ uint32_t coef[8 * TP], work[8 * TP];
  const uint32_t L = 1u << log_l, log_n = log_l + log_b, n_mask = (1u << log_n) - 1;
  const size_t row0 = (size_t)blockIdx.x << (LOG_T - log_l);
  for (uint32_t q = threadIdx.x; q < T; q += blockDim.x) {
    const uint32_t v = q >> log_l, j = q & (L - 1);
    Fr x = Fr::zero();
    if (row0 + v < num_rows) x = rows[(row0 + v) * cw + j];
    rs_st(coef, TP, (v << log_l) | rs_rev(j, log_l), x);
  }
  rs_tile_ntt(coef, TP, LOG_T, log_l, tw, log_n, true);
  for (uint32_t i = 1; i < (1u << log_b); i++) {
    for (uint32_t q = threadIdx.x; q < T; q += blockDim.x) {
      const uint32_t v = q >> log_l, t = q & (L - 1), e = (i * t) & n_mask;
      Fr x = rs_ld(coef, TP, q);
      if (log_l) x = mul(x, k_inv);
      if (e) x = mul(x, tw[e]);
      rs_st(work, TP, (v << log_l) | rs_rev(t, log_l), x);
    }
    rs_tile_ntt(work, TP, LOG_T, log_l, tw, log_n, false);
    for (uint32_t q = threadIdx.x; q < T; q += blockDim.x) {
      const uint32_t v = q >> log_l, j = q & (L - 1);
      if (row0 + v < num_rows) rows[(row0 + v) * cw + ((size_t)i << log_l) + j] = rs_ld(work, TP, q);
    }
    __syncthreads();  // (the next coset overwrites `work`)
  }
}

// ------------------------------------------------------------------ long rows: one pass of the four steps
struct RsPass {
  Fr* rows;
  const Fr* tw;
  size_t cw, num_vecs;         // vectors over all rows: num_rows << log_v
  size_t src_off, dst_off;     // within a row, for blockIdx.y = 0
  size_t src_step, dst_step;   // added per blockIdx.y (a coset per y)
  uint32_t log_l, log_v;       // vectors of 2^log_l elements, 2^log_v of them per row
  uint32_t log_n, log_b;
  uint32_t column;             // 1: vector u at +u, its element j at + j << log_v; 0: vector u at + u << log_l, contiguous
  uint32_t inverse;
  uint32_t coset;              // != 0: element t = u + (j << log_v) times w_N^((coset + blockIdx.y) t) going in
  uint32_t post_tw;            // output j' of vector u times w_K^(+- u j') coming out
  uint32_t has_scale;
  Fr scale;
};
__global__ void __launch_bounds__(RS_MAX_THREADS) bd_rs_pass_kernel(const RsPass a) {
  constexpr uint32_t T = 1u << RS_MAX_LOG_TILE, TP = T + (T >> 6);
  __shared__ uint32_t tile[8 * TP];
  const uint32_t log_c = RS_MAX_LOG_TILE - a.log_l, L = 1u << a.log_l, C = 1u << log_c;
  const uint64_t n_mask = ((uint64_t)1 << a.log_n) - 1;
  const size_t vec0 = (size_t)blockIdx.x << log_c, V = (size_t)1 << a.log_v;
  const size_t vstride = a.column ? 1 : L, estride = a.column ? V : 1;
  const Fr* src = a.rows + a.src_off + blockIdx.y * a.src_step;
  Fr* dst = a.rows + a.dst_off + blockIdx.y * a.dst_step;
  const uint64_t coset = a.coset ? a.coset + blockIdx.y : 0;
  for (uint32_t q = threadIdx.x; q < T; q += blockDim.x) {
    const uint32_t v = a.column ? q & (C - 1) : q >> a.log_l, j = a.column ? q >> log_c : q & (L - 1);
    const size_t g = vec0 + v;
    Fr x = Fr::zero();
    if (g < a.num_vecs) {
      const size_t row = g >> a.log_v, u = g & (V - 1);
      x = src[row * a.cw + u * vstride + j * estride];
      const uint64_t e = (coset * (u + ((uint64_t)j << a.log_v))) & n_mask;
      if (e) x = mul(x, a.tw[e]);
    }
    rs_st(tile, TP, (v << a.log_l) | rs_rev(j, a.log_l), x);
  }
  rs_tile_ntt(tile, TP, RS_MAX_LOG_TILE, a.log_l, a.tw, a.log_n, a.inverse != 0);
  for (uint32_t q = threadIdx.x; q < T; q += blockDim.x) {
    const uint32_t v = a.column ? q & (C - 1) : q >> a.log_l, j = a.column ? q >> log_c : q & (L - 1);
    const size_t g = vec0 + v;
    if (g >= a.num_vecs) continue;
    const size_t row = g >> a.log_v, u = g & (V - 1);
    Fr x = rs_ld(tile, TP, (v << a.log_l) | j);
    if (a.post_tw) {
      uint64_t e = ((uint64_t)u * j) << a.log_b;  // w_K = w_N^(2^b)
      if (a.inverse) e = (0 - e) & n_mask;
      if (e) x = mul(x, a.tw[e]);
    }
    if (a.has_scale) x = mul(x, a.scale);
    dst[row * a.cw + u * vstride + j * estride] = x;
  }
}

static Fr rs_inv_pow2(size_t log2_v) {  // 2^-log2_v, Montgomery form
  const host::Fr h = host::Fr::from_u64((uint64_t)1 << log2_v).inv();
  Fr out;
  memcpy(&out, &h, sizeof(out));
  return out;
}

void k_bd_rs_encode(Ctx& c, Fr* rows, size_t num_rows, size_t cw, size_t row_vars, int log_inv_rate, const Fr* tw) {
  LH_REQUIRE(log_inv_rate >= 1 && log_inv_rate <= 3 && row_vars <= LIGERO_MAX_DEVICE_ROW_VARS &&
                 cw == ((size_t)1 << (row_vars + log_inv_rate)),
             LH_ERR_ARG, "ligero: the device encoder takes rows of up to 2^22 at rate 1/2, 1/4 or 1/8");
  LH_REQUIRE(rows && tw, LH_ERR_ARG, "ligero: null rows or twiddle table");
  if (!num_rows) return;
  const uint32_t k = (uint32_t)row_vars, b = (uint32_t)log_inv_rate;
  const size_t K = (size_t)1 << k, cosets = (size_t)1 << b;
  const double elems = (double)num_rows * K;
  ProfScope ps(c, "bd_rs_encode", 32.0 * elems * (cosets + 1), elems * cosets * (k / 2.0 + 2), elems * cosets);
  if (k <= (uint32_t)RS_MAX_LOG_TILE) {
    uint32_t log_rows = 0;
    while (log_rows < 10 && ((size_t)1 << log_rows) < num_rows) log_rows++;
    const uint32_t want = std::max(k, std::min(k + log_rows, 10u)), log_t = k == 11 ? 11 : want <= 8 ? 8 : 10;
    const size_t tiles = (num_rows + ((size_t)1 << (log_t - k)) - 1) >> (log_t - k);
    LH_REQUIRE(tiles < ((size_t)1 << 31), LH_ERR_ARG, "ligero: too many rows in one launch");
    const Fr k_inv = rs_inv_pow2(k);
    const dim3 grid((unsigned)tiles);
    if (log_t == 8)
      hipLaunchKernelGGL(bd_rs_rows_kernel<8>, grid, 128, 0, c.stream, rows, cw, num_rows, k, b, tw, k_inv);
    else if (log_t == 10)
      hipLaunchKernelGGL(bd_rs_rows_kernel<10>, grid, 512, 0, c.stream, rows, cw, num_rows, k, b, tw, k_inv);
    else
      hipLaunchKernelGGL(bd_rs_rows_kernel<11>, grid, 512, 0, c.stream, rows, cw, num_rows, k, b, tw, k_inv);
    return;
  }
  const uint32_t k1 = k / 2, k2 = k - k1;  // K = K1 K2, both within a tile
  const size_t last = (cosets - 1) * K;
  RsPass col{}, row{};
  col.rows = row.rows = rows, col.tw = row.tw = tw, col.cw = row.cw = cw;
  col.log_n = row.log_n = k + b, col.log_b = row.log_b = b;
  col.column = 1, col.log_l = k1, col.log_v = k2, col.num_vecs = num_rows << k2;
  row.column = 0, row.log_l = k2, row.log_v = k1, row.num_vecs = num_rows << k1;
  const size_t tiles = (num_rows << k) >> RS_MAX_LOG_TILE;  // (either pass: num_vecs >> (11 - log_l))
  LH_REQUIRE(tiles < ((size_t)1 << 31), LH_ERR_ARG, "ligero: too many rows in one launch");
  auto launch = [&](const RsPass& a, unsigned ny) {
    hipLaunchKernelGGL(bd_rs_pass_kernel, dim3((unsigned)tiles, ny), RS_MAX_THREADS, 0, c.stream, a);
  };
  {  // the coefficients, into the last coset
    RsPass a = col;
    a.inverse = 1, a.post_tw = 1, a.src_off = 0, a.dst_off = last, a.has_scale = 1, a.scale = rs_inv_pow2(k);
    launch(a, 1);
    a = row;
    a.inverse = 1, a.src_off = a.dst_off = last;
    launch(a, 1);
  }
  auto coset_passes = [&](uint32_t first, unsigned count) {
    RsPass a = row;
    a.coset = first, a.post_tw = 1, a.src_off = last, a.dst_off = first * K, a.dst_step = K;
    launch(a, count);
    a = col;
    a.src_off = a.dst_off = first * K, a.src_step = a.dst_step = K;
    launch(a, count);
  };
  if (cosets > 2) coset_passes(1, (unsigned)cosets - 2);
  coset_passes((uint32_t)cosets - 1, 1);
}

}  // namespace lh
