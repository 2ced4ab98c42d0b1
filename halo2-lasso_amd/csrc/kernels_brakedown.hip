// Kernels of the Brakedown PCS (reference util/code/brakedown.rs:88-125, pcs/multilinear/brakedown.rs:130-276).
//   bd_gather        one sparse-matrix stage of the encoder, all rows at once: out[j] = sum_e in[idx[e]] val[e] over the
//                    transposed CSR group of output j (a gather: no atomics, a fixed summation order)
//   bd_reed_solomon  the cascade's tail, one workgroup per row: tmp = a_last . in in LDS, then horner(tmp, x), x = 1, 2, ..
//   bd_hash_columns  keccak256(to_repr(rows[0][c]) || .. || to_repr(rows[R-1][c])), one thread per column, the state in
//                    registers; leaves from codeword_len up to 2^depth are zero
//   bd_merkle_level  parent = keccak256(left || right)
//   bd_combine       the proximity row(s) and the t_0 row in one pass over the polynomial
// A batch of P polys (brakedown_batch_commit) is one slab of P * num_rows rows: the encoder stages above take it as it is
// (rows are independent), and what is per poly gets blockIdx.y = poly:
//   bd_load_rows           the P messages from a pointer table into the slab's rows
//   bd_hash_columns_batch  / bd_merkle_level_batch: the same leaves and parents, poly p's tree at p * tree_stride
//   bd_stage_columns       the encoded matrix transposed (column-major) through LDS tiles, for the staged open
// A batch of COLUMNS (brakedown_commit_columns: Lasso's u32 witness columns, `len` entries, zero beyond) has a table of
// (pointer, len, kind) in device memory, blockIdx.y = column:
//   bd_load_columns        the messages into the slab's rows: u32 entries converted to Montgomery form, Fr entries copied,
//                          zero from `len` on (an all-padding row is a zero message and encodes to a zero row)
//   bd_gather_u32          the first forward stage a[0] from the 4-byte entries themselves: val[e] * x as a 256 x 32-bit
//                          product of the Montgomery-form coefficient and the plain integer, a group's sum unreduced in
//                          ten limbs (wide.cuh), one reduction per output to the canonical Montgomery value bd_gather stores
#include <hip/hip_runtime.h>
#include "brakedown.hpp"
#include "launch.cuh"
#include "wide.cuh"

namespace lh {

constexpr size_t BD_GRID_CAP = 8192;  // (the cap of this file's element-wise launches)

// ------------------------------------------------------------------ encoder stages
__global__ void bd_gather_kernel(Fr* __restrict__ rows, size_t num_rows, size_t cw, size_t in_off, size_t out_off,
                                 size_t m, const uint32_t* __restrict__ ptr, const uint32_t* __restrict__ idx,
                                 const Fr* __restrict__ val) {
  GSTRIDE(t, num_rows * m) {
    const size_t r = t / m, j = t - r * m;
    const Fr* in = rows + r * cw + in_off;
    Fr acc = Fr::zero();
    for (uint32_t e = ptr[j], end = ptr[j + 1]; e < end; e++) acc = add(acc, mul(in[idx[e]], val[e]));
    rows[r * cw + out_off + j] = acc;
  }
}
void k_bd_gather(Ctx& c, Fr* rows, size_t num_rows, size_t cw, size_t in_off, size_t out_off, const BdMatrix& mat) {
  const size_t m = mat.dim.m;
  if (!m || !num_rows) return;
  ProfScope ps(c, "bd_gather", 64.0 * num_rows * mat.dim.n * mat.dim.d, (double)num_rows * mat.dim.n * mat.dim.d,
               (double)num_rows * m);
  hipLaunchKernelGGL(bd_gather_kernel, grid_for(num_rows * m, 256, BD_GRID_CAP), 256, 0, c.stream, rows, num_rows, cw, in_off, out_off, m,
                     mat.d_ptr, mat.d_idx, mat.d_val);
}

// ------------------------------------------------------------------ a[0] of u32 columns
// bd_gather on the loaded message computes sum_e mont(x_e) * val[e] = (sum_e x_e v_e) mod r as an integer, v_e the limbs of
// val[e] (V_e R mod r) and x_e the plain entries.  Here the integer sum itself is formed with wide.cuh's accumulator (8
// multiply-adds per term into ten limbs: a term is below 2^32 r < 2^286 and a group has fewer than 2^32 of them - the CSR
// index type - so the sum is below 2^318) and reduced once per output by wide_reduce, whose result is the canonical value
// in [0, r): bit for bit what bd_gather stores.
__global__ void bd_gather_u32_kernel(const BdColumn* __restrict__ cols, Fr* __restrict__ rows, size_t num_rows,
                                     size_t row_len, size_t cw, size_t m, const uint32_t* __restrict__ ptr,
                                     const uint32_t* __restrict__ idx, const Fr* __restrict__ val) {
  const BdColumn col = cols[blockIdx.y];
  if (!col.u32) return;  // (a field-element column keeps bd_gather)
  const uint32_t* __restrict__ x = (const uint32_t*)col.data;
  Fr* dst = rows + (size_t)blockIdx.y * num_rows * cw;
  GSTRIDE(t, num_rows * m) {
    const size_t r = t / m, j = t - r * m, base = r * row_len;
    Wide s = Wide::zero();
    for (uint32_t e = ptr[j], end = ptr[j + 1]; e < end; e++) {
      const size_t k = base + idx[e];
      if (k >= col.len) continue;  // the zero padding: nothing is read past `len`
      wide_mac(s, val[e], x[k]);
    }
    dst[r * cw + row_len + j] = wide_reduce(s);
  }
}
constexpr size_t BD_MAX_BATCH = 65535;  // gridDim.y
void k_bd_gather_u32(Ctx& c, const BdColumn* d_cols, size_t num_cols, Fr* rows, size_t num_rows, size_t row_len, size_t cw,
                     const BdMatrix& mat) {
  const size_t m = mat.dim.m;
  LH_REQUIRE(num_cols >= 1 && num_cols <= BD_MAX_BATCH, LH_ERR_ARG, "brakedown: too many columns in one batch");
  LH_REQUIRE(mat.dim.n == row_len && row_len + m <= cw, LH_ERR_ARG, "brakedown: not the first stage's matrix");
  if (!m || !num_rows) return;
  ProfScope ps(c, "bd_gather_u32", 40.0 * num_cols * num_rows * mat.dim.n * mat.dim.d,
               (double)num_cols * num_rows * mat.dim.n * mat.dim.d / 8, (double)num_cols * num_rows * m);
  dim3 g = grid_for(num_rows * m, 256, BD_GRID_CAP);
  g.y = (unsigned)num_cols;
  hipLaunchKernelGGL(bd_gather_u32_kernel, g, 256, 0, c.stream, d_cols, rows, num_rows, row_len, cw, m, mat.d_ptr,
                     mat.d_idx, mat.d_val);
}

constexpr int BD_RS_MAX = 64;  // a_last.m <= n_0 <= 20 (dimensions stop at n <= n_0)
__global__ void bd_reed_solomon_kernel(Fr* __restrict__ rows, size_t cw, size_t in_off, size_t an, size_t am, size_t bn,
                                       const uint32_t* __restrict__ ptr, const uint32_t* __restrict__ idx,
                                       const Fr* __restrict__ val) {
  __shared__ Fr tmp[BD_RS_MAX];
  Fr* row = rows + (size_t)blockIdx.x * cw;
  const Fr* in = row + in_off;
  for (size_t j = threadIdx.x; j < am; j += blockDim.x) {
    Fr acc = Fr::zero();
    for (uint32_t e = ptr[j], end = ptr[j + 1]; e < end; e++) acc = add(acc, mul(in[idx[e]], val[e]));
    tmp[j] = acc;
  }
  __syncthreads();
  for (size_t x = threadIdx.x; x < bn; x += blockDim.x) {
    const Fr xv = from_u64<FrParams>(x + 1);
    Fr acc = Fr::zero();
    for (size_t k = am; k-- > 0;) acc = add(mul(acc, xv), tmp[k]);
    row[in_off + an + x] = acc;
  }
}
void k_bd_reed_solomon(Ctx& c, Fr* rows, size_t num_rows, size_t cw, size_t in_off, const BdMatrix& a_last, size_t bn) {
  LH_REQUIRE(a_last.dim.m <= (size_t)BD_RS_MAX, LH_ERR_ARG, "brakedown: Reed-Solomon message too long");
  if (!num_rows) return;
  ProfScope ps(c, "bd_reed_solomon", 64.0 * num_rows * (a_last.dim.n * a_last.dim.d + bn * a_last.dim.m),
               (double)num_rows * (a_last.dim.n * a_last.dim.d + bn * a_last.dim.m), (double)num_rows * bn);
  hipLaunchKernelGGL(bd_reed_solomon_kernel, dim3((unsigned)num_rows), 64, 0, c.stream, rows, cw, in_off, a_last.dim.n,
                     a_last.dim.m, bn, a_last.d_ptr, a_last.d_idx, a_last.d_val);
}

// ------------------------------------------------------------------ Keccak-f[1600], the 25 lanes in registers
__constant__ uint64_t BD_RC[24] = {
    0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808Aull, 0x8000000080008000ull,
    0x000000000000808Bull, 0x0000000080000001ull, 0x8000000080008081ull, 0x8000000000008009ull,
    0x000000000000008Aull, 0x0000000000000088ull, 0x0000000080008009ull, 0x000000008000000Aull,
    0x000000008000808Bull, 0x800000000000008Bull, 0x8000000000008089ull, 0x8000000000008003ull,
    0x8000000000008002ull, 0x8000000000000080ull, 0x000000000000800Aull, 0x800000008000000Aull,
    0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};

__device__ __forceinline__ uint64_t rotl64(uint64_t v, int n) { return n ? (v << n) | (v >> (64 - n)) : v; }

// every array index below is a compile-time constant once the loops are unrolled: the state never leaves registers
__device__ __forceinline__ void keccak_f1600(uint64_t (&a)[25]) {
  constexpr int RHO[25] = {0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14};
#pragma unroll 1
  for (int rnd = 0; rnd < 24; rnd++) {
    uint64_t c[5], b[25];
#pragma unroll
    for (int x = 0; x < 5; x++) c[x] = a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20];
#pragma unroll
    for (int x = 0; x < 5; x++) {
      const uint64_t d = c[(x + 4) % 5] ^ rotl64(c[(x + 1) % 5], 1);
#pragma unroll
      for (int y = 0; y < 5; y++) b[y + 5 * ((2 * x + 3 * y) % 5)] = rotl64(a[x + 5 * y] ^ d, RHO[x + 5 * y]);
    }
#pragma unroll
    for (int y = 0; y < 5; y++)
#pragma unroll
      for (int x = 0; x < 5; x++) a[x + 5 * y] = b[x + 5 * y] ^ (~b[(x + 1) % 5 + 5 * y] & b[(x + 2) % 5 + 5 * y]);
    a[0] ^= BD_RC[rnd];
  }
}

__device__ __forceinline__ void store_digest(uint64_t* out, const uint64_t (&a)[25]) {
  ulonglong2* o = (ulonglong2*)out;  // two 16-byte vector stores
  o[0] = make_ulonglong2(a[0], a[1]);
  o[1] = make_ulonglong2(a[2], a[3]);
}

// Column c's message is num_rows elements of 4 words; 17 elements = 68 words = exactly 4 rate blocks of 17 lanes, so with
// the block's place in its group of 17 elements (BI) a template parameter every word's lane is a compile-time constant.
// `cnt` elements of the group are data; on the last group the padding follows them (0x01 after the data, 0x80 in the last
// byte of the padding block).  An element that straddles two blocks is loaded by both.
template <int BI>
__device__ __forceinline__ void bd_absorb_block(uint64_t (&a)[25], const Fr* col, size_t cw, int cnt, bool last,
                                                bool pad_block) {
  constexpr int first = 17 * BI, k0 = first / 4, k1 = (first + 16) / 4;
#pragma unroll
  for (int k = k0; k <= k1; k++) {
    uint64_t w[4] = {0, 0, 0, 0};
    if (k < cnt) {
      const Fr v = from_mont(col[(size_t)k * cw]);  // to_repr: canonical, little-endian
#pragma unroll
      for (int t = 0; t < 4; t++) w[t] = (uint64_t)v.l[2 * t] | ((uint64_t)v.l[2 * t + 1] << 32);
    }
#pragma unroll
    for (int t = 0; t < 4; t++) {
      const int pos = 4 * k + t;
      if (pos < first || pos > first + 16) continue;
      uint64_t v = w[t];
      if (last && pos == 4 * cnt) v ^= 0x01ull;
      a[pos - first] ^= v;
    }
  }
  if (pad_block) a[16] ^= 0x80ull << 56;
}

// (64-thread workgroups: the state, the permutation's temporaries and a Montgomery product fit without spilling)
__device__ __forceinline__ void bd_hash_columns_body(const Fr* __restrict__ rows, size_t num_rows, size_t cw, size_t width,
                                                     uint64_t* __restrict__ leaves) {
  GSTRIDE(c, width) {
    uint64_t a[25];
#pragma unroll
    for (int i = 0; i < 25; i++) a[i] = 0;
    if (c < cw) {
      const size_t full = num_rows / 17;
      for (size_t g = 0; g <= full; g++) {
        const Fr* col = rows + g * 17 * cw + c;
        const bool last = g == full;
        const int cnt = last ? (int)(num_rows - full * 17) : 17, pad = (4 * cnt) / 17, nblk = last ? pad + 1 : 4;
#pragma unroll 1
        for (int bi = 0; bi < nblk; bi++) {
          const bool pb = last && bi == pad;
          switch (bi) {
            case 0: bd_absorb_block<0>(a, col, cw, cnt, last, pb); break;
            case 1: bd_absorb_block<1>(a, col, cw, cnt, last, pb); break;
            case 2: bd_absorb_block<2>(a, col, cw, cnt, last, pb); break;
            default: bd_absorb_block<3>(a, col, cw, cnt, last, pb); break;
          }
          keccak_f1600(a);
        }
      }
    }
    store_digest(leaves + 4 * c, a);  // (the zero leaves past codeword_len: a is still all zero)
  }
}
__global__ void __launch_bounds__(64)
    bd_hash_columns_kernel(const Fr* __restrict__ rows, size_t num_rows, size_t cw, size_t width, uint64_t* __restrict__ leaves) {
  bd_hash_columns_body(rows, num_rows, cw, width, leaves);
}
// poly blockIdx.y of a slab: its rows at y * num_rows * cw, its tree at y * tree_stride words
__global__ void __launch_bounds__(64)
    bd_hash_columns_batch_kernel(const Fr* __restrict__ rows, size_t num_rows, size_t cw, size_t width,
                                 uint64_t* __restrict__ trees, size_t tree_stride) {
  bd_hash_columns_body(rows + (size_t)blockIdx.y * num_rows * cw, num_rows, cw, width, trees + (size_t)blockIdx.y * tree_stride);
}
void k_bd_hash_columns(Ctx& c, const Fr* rows, size_t num_rows, size_t cw, size_t width, uint64_t* leaves) {
  ProfScope ps(c, "bd_hash_columns", 32.0 * num_rows * cw + 32.0 * width, 0, (double)cw);
  hipLaunchKernelGGL(bd_hash_columns_kernel, grid_for(width, 64, 1 << 16), 64, 0, c.stream, rows, num_rows, cw, width,
                     leaves);
}

__device__ __forceinline__ void bd_merkle_level_body(const uint64_t* __restrict__ in, size_t out_n, uint64_t* __restrict__ out) {
  GSTRIDE(i, out_n) {
    uint64_t a[25];
    const ulonglong2* src = (const ulonglong2*)(in + 8 * i);
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const ulonglong2 v = src[k];
      a[2 * k] = v.x, a[2 * k + 1] = v.y;
    }
#pragma unroll
    for (int k = 8; k < 25; k++) a[k] = 0;
    a[8] = 0x01ull;
    a[16] = 0x80ull << 56;
    keccak_f1600(a);
    store_digest(out + 4 * i, a);
  }
}
__global__ void __launch_bounds__(64)
    bd_merkle_level_kernel(const uint64_t* __restrict__ in, size_t out_n, uint64_t* __restrict__ out) {
  bd_merkle_level_body(in, out_n, out);
}
__global__ void __launch_bounds__(64)
    bd_merkle_level_batch_kernel(uint64_t* __restrict__ trees, size_t tree_stride, size_t in_off, size_t out_n, size_t out_off) {
  uint64_t* tree = trees + (size_t)blockIdx.y * tree_stride;
  bd_merkle_level_body(tree + in_off, out_n, tree + out_off);
}
void k_bd_merkle_level(Ctx& c, const uint64_t* in, size_t out_n, uint64_t* out) {
  ProfScope ps(c, "bd_merkle_level", 96.0 * out_n, 0, (double)out_n);
  hipLaunchKernelGGL(bd_merkle_level_kernel, grid_for(out_n, 64, 1 << 16), 64, 0, c.stream, in, out_n, out);
}

// ------------------------------------------------------------------ a batch of polys in one slab
__global__ void bd_load_rows_kernel(const Fr* const* __restrict__ polys, size_t num_rows, size_t row_len, size_t cw,
                                    Fr* __restrict__ rows) {
  const Fr* __restrict__ src = polys[blockIdx.y];
  Fr* dst = rows + (size_t)blockIdx.y * num_rows * cw;
  GSTRIDE(t, num_rows * row_len) {
    const size_t r = t / row_len, j = t - r * row_len;
    dst[r * cw + j] = src[t];  // row r's message is poly[r * row_len ..]
  }
}
void k_bd_load_rows(Ctx& c, const Fr* const* d_polys, size_t num_polys, size_t num_rows, size_t row_len, size_t cw, Fr* rows) {
  LH_REQUIRE(num_polys >= 1 && num_polys <= BD_MAX_BATCH, LH_ERR_ARG, "brakedown: too many polys in one batch");
  ProfScope ps(c, "bd_load_rows", 64.0 * num_polys * num_rows * row_len, 0, (double)num_polys * num_rows * row_len);
  dim3 g = grid_for(num_rows * row_len, 256, BD_GRID_CAP);
  g.y = (unsigned)num_polys;
  hipLaunchKernelGGL(bd_load_rows_kernel, g, 256, 0, c.stream, d_polys, num_rows, row_len, cw, rows);
}
__global__ void bd_load_columns_kernel(const BdColumn* __restrict__ cols, size_t num_rows, size_t row_len, size_t cw,
                                       Fr* __restrict__ rows) {
  const BdColumn col = cols[blockIdx.y];
  Fr* dst = rows + (size_t)blockIdx.y * num_rows * cw;
  GSTRIDE(t, num_rows * row_len) {
    const size_t r = t / row_len, j = t - r * row_len;
    Fr v = Fr::zero();
    if (t < col.len) {
      if (col.u32) {
        const uint32_t x = ((const uint32_t*)col.data)[t];
        if (x) v = from_u64<FrParams>(x);
      } else {
        v = ((const Fr*)col.data)[t];
      }
    }
    dst[r * cw + j] = v;
  }
}
void k_bd_load_columns(Ctx& c, const BdColumn* d_cols, size_t num_cols, size_t num_rows, size_t row_len, size_t cw, Fr* rows) {
  LH_REQUIRE(num_cols >= 1 && num_cols <= BD_MAX_BATCH, LH_ERR_ARG, "brakedown: too many columns in one batch");
  ProfScope ps(c, "bd_load_columns", 36.0 * num_cols * num_rows * row_len, (double)num_cols * num_rows * row_len,
               (double)num_cols * num_rows * row_len);
  dim3 g = grid_for(num_rows * row_len, 256, BD_GRID_CAP);
  g.y = (unsigned)num_cols;
  hipLaunchKernelGGL(bd_load_columns_kernel, g, 256, 0, c.stream, d_cols, num_rows, row_len, cw, rows);
}
void k_bd_hash_columns_batch(Ctx& c, const Fr* rows, size_t num_polys, size_t num_rows, size_t cw, size_t width,
                             uint64_t* trees, size_t tree_stride) {
  LH_REQUIRE(num_polys >= 1 && num_polys <= BD_MAX_BATCH, LH_ERR_ARG, "brakedown: too many polys in one batch");
  ProfScope ps(c, "bd_hash_columns", num_polys * (32.0 * num_rows * cw + 32.0 * width), 0, (double)num_polys * cw);
  dim3 g = grid_for(width, 64, 1 << 16);
  g.y = (unsigned)num_polys;
  hipLaunchKernelGGL(bd_hash_columns_batch_kernel, g, 64, 0, c.stream, rows, num_rows, cw, width, trees, tree_stride);
}
void k_bd_merkle_level_batch(Ctx& c, uint64_t* trees, size_t num_polys, size_t tree_stride, size_t in_off, size_t out_n,
                             size_t out_off) {
  LH_REQUIRE(num_polys >= 1 && num_polys <= BD_MAX_BATCH, LH_ERR_ARG, "brakedown: too many polys in one batch");
  ProfScope ps(c, "bd_merkle_level", 96.0 * num_polys * out_n, 0, (double)num_polys * out_n);
  dim3 g = grid_for(out_n, 64, 1 << 16);
  g.y = (unsigned)num_polys;
  hipLaunchKernelGGL(bd_merkle_level_batch_kernel, g, 64, 0, c.stream, trees, tree_stride, in_off, out_n, out_off);
}
__global__ void bd_gather_roots_kernel(const uint64_t* __restrict__ trees, size_t tree_stride, size_t root_off,
                                       size_t num_polys, uint64_t* __restrict__ out) {
  GSTRIDE(t, 4 * num_polys) out[t] = trees[(t / 4) * tree_stride + root_off + (t & 3)];
}
void k_bd_gather_roots(Ctx& c, const uint64_t* trees, size_t num_polys, size_t tree_stride, size_t root_off, uint64_t* out) {
  hipLaunchKernelGGL(bd_gather_roots_kernel, grid_for(4 * num_polys, 256, BD_GRID_CAP), 256, 0, c.stream, trees, tree_stride, root_off,
                     num_polys, out);
}

// ------------------------------------------------------------------ staged open: the encoded matrix, column-major
// out[c * num_rows + r] = rows[r * cw + c].  A workgroup moves a tile of BD_T x BD_T elements through the LDS: lane (ty, tx)
// loads element (row r0 + ty, column c0 + tx) - adjacent lanes read adjacent 32-byte elements of a row - and stores element
// (column c0 + ty, row r0 + tx) - adjacent lanes write adjacent elements of a column.  An element is two 16-byte halves
// (ds_write_b128 / ds_read_b128).  A tile row is BD_T elements plus one 16-byte pad: without it the transposed read of a
// 16-lane group walks a stride of 512 bytes, two bank rows of 256, and the lanes that share a tile column land on the same
// four banks (8-way); with the pad the stride is 33 slots of 16 bytes and the slots differ (slot = r + 2 c + half mod 16: at
// worst two pairs of lanes meet, where a group spans two tile columns).  The row-wise store is 2-way (ds_write_b128 banks
// modulo 128 bytes, a lane every 32).  Each byte crosses HBM once in and once out, far below what the LDS carries even so.
// Edge tiles: lanes beyond num_rows or cw neither load nor store.
constexpr int BD_T = 16;
constexpr int BD_T_STRIDE = 2 * BD_T + 1;  // 16-byte slots per tile row
__global__ void __launch_bounds__(BD_T * BD_T)
    bd_stage_columns_kernel(const Fr* __restrict__ rows, size_t num_rows, size_t cw, Fr* __restrict__ out) {
  __shared__ uint4 tile[BD_T * BD_T_STRIDE];
  const int tx = threadIdx.x % BD_T, ty = threadIdx.x / BD_T;
  const size_t c0 = (size_t)blockIdx.x * BD_T, r0 = (size_t)blockIdx.y * BD_T;
  if (r0 + ty < num_rows && c0 + tx < cw) {
    const uint4* src = (const uint4*)(rows + (r0 + ty) * cw + c0 + tx);
    tile[ty * BD_T_STRIDE + 2 * tx] = src[0];
    tile[ty * BD_T_STRIDE + 2 * tx + 1] = src[1];
  }
  __syncthreads();
  if (c0 + ty < cw && r0 + tx < num_rows) {
    uint4* dst = (uint4*)(out + (c0 + ty) * num_rows + r0 + tx);
    dst[0] = tile[tx * BD_T_STRIDE + 2 * ty];
    dst[1] = tile[tx * BD_T_STRIDE + 2 * ty + 1];
  }
}
void k_bd_stage_columns(Ctx& c, const Fr* rows, size_t num_rows, size_t cw, Fr* out) {
  const size_t gx = (cw + BD_T - 1) / BD_T, gy = (num_rows + BD_T - 1) / BD_T;
  LH_REQUIRE(num_rows >= 1 && cw >= 1 && gx < ((size_t)1 << 31) && gy <= 65535, LH_ERR_ARG,
             "brakedown: matrix too large to stage");
  ProfScope ps(c, "bd_stage_columns", 64.0 * num_rows * cw, 0, (double)num_rows * cw);
  hipLaunchKernelGGL(bd_stage_columns_kernel, dim3((unsigned)gx, (unsigned)gy), BD_T * BD_T, 0, c.stream, rows, num_rows, cw,
                     out);
}

// ------------------------------------------------------------------ open: combined rows
constexpr int BD_MAX_SETS = 4;
__global__ void bd_combine_kernel(const Fr* __restrict__ poly, size_t num_rows, size_t row_len, size_t stride,
                                  const Fr* __restrict__ coeffs, int num_sets, Fr* __restrict__ out) {
  GSTRIDE(col, row_len) {
    Fr acc[BD_MAX_SETS];
#pragma unroll
    for (int k = 0; k < BD_MAX_SETS; k++) acc[k] = Fr::zero();
    for (size_t r = 0; r < num_rows; r++) {
      const Fr x = poly[r * stride + col];
#pragma unroll
      for (int k = 0; k < BD_MAX_SETS; k++)
        if (k < num_sets) acc[k] = add(acc[k], mul(coeffs[k * num_rows + r], x));
    }
#pragma unroll
    for (int k = 0; k < BD_MAX_SETS; k++)
      if (k < num_sets) out[k * row_len + col] = acc[k];
  }
}
void k_bd_combine(Ctx& c, const Fr* poly, size_t num_rows, size_t row_len, size_t stride, const Fr* coeffs, int num_sets,
                  Fr* out) {
  LH_REQUIRE(num_sets >= 1 && num_sets <= BD_MAX_SETS, LH_ERR_ARG, "brakedown: too many combinations in one pass");
  ProfScope ps(c, "bd_combine", 32.0 * num_rows * row_len, (double)num_sets * num_rows * row_len, (double)row_len);
  hipLaunchKernelGGL(bd_combine_kernel, grid_for(row_len, 256, BD_GRID_CAP), 256, 0, c.stream, poly, num_rows, row_len, stride, coeffs,
                     num_sets, out);
}

}  // namespace lh
