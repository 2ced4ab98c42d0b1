// Kernels of the multilinear IPA over BN254 G1 (reference pcs/multilinear/ipa.rs:98-241).
//   generators   g[idx] of the library's own hash-to-point (Keccak-256 of domain || message || counter || tag twice, a
//                512-bit integer reduced mod q, the square root by one exponentiation): one thread per generator
//   base fold    out[j] = a[j] + s b[j] for ONE scalar s shared by every thread, back in affine form.  The digits of s
//                (non-adjacent form, made on the host) are uniform over the launch: the double-and-add branches on kernel
//                arguments alone, and only the exceptional cases of the additions diverge.  The sums are left in XYZZ and
//                a second launch normalises them, AX_BATCH points per thread behind one inversion; an identity among them
//                takes the place of a one in the running product and comes out as (0, 0).
//   cross        <coeffs_r, zs_l> and <coeffs_l, zs_r> of a round in one pass
//   fold_fr      coeffs_l += xi^-1 coeffs_r and zs_l += xi zs_r in one launch
#include <hip/hip_runtime.h>
#include <algorithm>
#include "dev.hpp"
#include "ff_host.hpp"
#include "launch.cuh"
#include "reduce.cuh"

namespace lh {

static inline unsigned blocks_for(size_t n, size_t block, size_t cap) {
  size_t g = (n + block - 1) / block;
  return (unsigned)(g < 1 ? 1 : g > cap ? cap : g);
}

// ------------------------------------------------------------------ generators
__constant__ uint64_t IPA_RC[24] = {
    0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808Aull, 0x8000000080008000ull,
    0x000000000000808Bull, 0x0000000080000001ull, 0x8000000080008081ull, 0x8000000000008009ull,
    0x000000000000008Aull, 0x0000000000000088ull, 0x0000000080008009ull, 0x000000008000000Aull,
    0x000000008000808Bull, 0x800000000000008Bull, 0x8000000000008089ull, 0x8000000000008003ull,
    0x8000000000008002ull, 0x8000000000000080ull, 0x000000000000800Aull, 0x800000008000000Aull,
    0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};

__device__ __forceinline__ uint64_t ipa_rotl(uint64_t v, int n) { return n ? (v << n) | (v >> (64 - n)) : v; }

__device__ __forceinline__ void ipa_keccak_f(uint64_t (&a)[25]) {
  constexpr int RHO[25] = {0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14};
#pragma unroll 1
  for (int rnd = 0; rnd < 24; rnd++) {
    uint64_t c[5], b[25];
#pragma unroll
    for (int x = 0; x < 5; x++) c[x] = a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20];
#pragma unroll
    for (int x = 0; x < 5; x++) {
      const uint64_t d = c[(x + 4) % 5] ^ ipa_rotl(c[(x + 1) % 5], 1);
#pragma unroll
      for (int y = 0; y < 5; y++) b[y + 5 * ((2 * x + 3 * y) % 5)] = ipa_rotl(a[x + 5 * y] ^ d, RHO[x + 5 * y]);
    }
#pragma unroll
    for (int y = 0; y < 5; y++)
#pragma unroll
      for (int x = 0; x < 5; x++) a[x + 5 * y] = b[x + 5 * y] ^ (~b[(x + 1) % 5 + 5 * y] & b[(x + 2) % 5 + 5 * y]);
    a[0] ^= IPA_RC[rnd];
  }
}

// a 256-bit integer (< 6 q) -> the field element, Montgomery form
__device__ __forceinline__ Fq ipa_fq_from_u256(Fq v) {
#pragma unroll 1
  for (int k = 0; k < 5; k++) {
    Fq t;
    uint64_t bw = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const uint64_t d = (uint64_t)v.l[i] - FqParams::mod(i) - bw;
      t.l[i] = (uint32_t)d;
      bw = d >> 63;
    }
    if (!bw) v = t;
  }
  return to_mont(v);
}

// the message of g[idx] is 31 bytes, one rate block: the 21 bytes of the domain, 0x00, le32(idx), le32(ctr), the tag byte;
// the padding's 0x01 is byte 31 and its 0x80 byte 135 (lane 16).  d0 / d1 -> the limbs of the 512-bit integer.
struct IpaDomain {
  uint64_t lane0, lane1, lane2;  // bytes 0..20 of the block (lane2: its low 5 bytes)
};
__device__ __forceinline__ void ipa_digest(const IpaDomain& dm, uint32_t idx, uint32_t ctr, uint32_t tag, Fq& out) {
  uint64_t a[25];
#pragma unroll
  for (int i = 0; i < 25; i++) a[i] = 0;
  a[0] = dm.lane0, a[1] = dm.lane1;
  a[2] = dm.lane2 | ((uint64_t)(idx & 0xffffu) << 48);
  a[3] = (uint64_t)(idx >> 16) | ((uint64_t)ctr << 16) | ((uint64_t)tag << 48) | (0x01ull << 56);
  a[16] = 0x80ull << 56;
  ipa_keccak_f(a);
#pragma unroll
  for (int t = 0; t < 4; t++) out.l[2 * t] = (uint32_t)a[t], out.l[2 * t + 1] = (uint32_t)(a[t] >> 32);
}

__global__ __launch_bounds__(128) void ipa_generators_kernel(IpaDomain dm, uint32_t first, size_t n, G1Affine* __restrict__ out) {
  uint32_t e[8];  // (q + 1) / 4
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint32_t lo = FqParams::mod(i) + (i == 0 ? 1u : 0u), hi = i < 7 ? FqParams::mod(i + 1) : 0u;
    e[i] = (lo >> 2) | (hi << 30);
  }
  const Fq three = from_u64<FqParams>(3);
  GSTRIDE(j, n) {
    const uint32_t idx = first + (uint32_t)j;
    G1Affine p;
    for (uint32_t ctr = 0;; ctr++) {
      Fq d0, d1;
      ipa_digest(dm, idx, ctr, 0, d0);
      ipa_digest(dm, idx, ctr, 1, d1);
      // x = d0 + 2^256 d1: in Montgomery form 2^256 is the constant R^2 mod q
      const Fq x = add(ipa_fq_from_u256(d0), mul(ipa_fq_from_u256(d1), Fq::r2()));
      const Fq rhs = add(mul(sqr(x), x), three);
      Fq y = pow_limbs(rhs, e);
      if (y.is_zero() || sqr(y) != rhs) continue;
      if (from_mont(y).l[0] & 1u) y = neg(y);
      p.x = x, p.y = y;
      break;
    }
    out[j] = p;
  }
}

void k_ipa_generators(Ctx& c, size_t first, size_t n, G1Affine* out) {
  if (!n) return;
  ProfScope ps(c, "ipa_generators", 64.0 * n, 2.0 * 400 * n, (double)n);
  static const char domain[] = "MultilinearIpa::setup";
  static_assert(sizeof(domain) - 1 == 21, "domain length");
  uint8_t block[24] = {0};
  memcpy(block, domain, 21);
  IpaDomain dm;
  memcpy(&dm.lane0, block, 8), memcpy(&dm.lane1, block + 8, 8), memcpy(&dm.lane2, block + 16, 8);
  hipLaunchKernelGGL(ipa_generators_kernel, dim3(blocks_for(n, 128, 1 << 16)), dim3(128), 0, c.stream, dm, (uint32_t)first, n, out);
}

// ------------------------------------------------------------------ base fold
constexpr int AX_BATCH = 8;  // points behind one inversion
struct AxDigits {            // non-adjacent form of the shared scalar: digit i is +1 (pos), -1 (neg) or 0; digits above `top` are 0
  uint32_t pos[8], neg[8];
  int top;
};

__global__ __launch_bounds__(128) void g1_axpy_kernel(const G1Affine* __restrict__ a, const G1Affine* __restrict__ b, size_t n,
                                                      AxDigits s, G1Xyzz* __restrict__ sums) {
  GSTRIDE(j, n) {
    const G1Affine bj = b[j];
    G1Xyzz acc = G1Xyzz::identity();
    for (int i = s.top; i >= 0; i--) {  // (uniform: the digits are kernel arguments)
      acc = dbl(acc);
      const uint32_t p = (s.pos[i >> 5] >> (i & 31)) & 1u, m = (s.neg[i >> 5] >> (i & 31)) & 1u;
      if (p | m) acc = add_mixed(acc, bj, m != 0);
    }
    sums[j] = add_mixed(acc, a[j]);
  }
}

__global__ __launch_bounds__(128) void g1_normalize_kernel(const G1Xyzz* __restrict__ sums, size_t n, G1Affine* __restrict__ out) {
  const size_t groups = (n + AX_BATCH - 1) / AX_BATCH;
  GSTRIDE(g, groups) {
    const size_t i0 = g * AX_BATCH;
    Fq pre[AX_BATCH];
    Fq run = Fq::one();
#pragma unroll
    for (int k = 0; k < AX_BATCH; k++) {
      pre[k] = run;
      if (i0 + k < n) {
        const Fq zz = sums[i0 + k].zz;
        if (!zz.is_zero()) run = mul(run, mul(zz, sums[i0 + k].zzz));
      }
    }
    Fq iv = inv(run);  // (run is a product of nonzero elements: never zero)
#pragma unroll
    for (int k = AX_BATCH - 1; k >= 0; k--) {
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

void k_g1_axpy(Ctx& c, const G1Affine* a, const G1Affine* b, size_t n, const Fr& s, G1Affine* out) {
  if (!n) return;
  ProfScope ps(c, "ipa_base_fold", 192.0 * n, 3200.0 * n, (double)n);
  // non-adjacent form of the canonical scalar (< 2^254: at most 255 digits)
  AxDigits d;
  memset(&d, 0, sizeof d);
  d.top = -1;
  host::Fr hs;
  memcpy(&hs, &s, 32);
  uint64_t k[5] = {0, 0, 0, 0, 0};
  hs.to_canonical(k);
  for (int i = 0; i < 256 && (k[0] | k[1] | k[2] | k[3] | k[4]); i++) {
    if (k[0] & 1) {
      if ((k[0] & 3) == 1) {
        d.pos[i >> 5] |= 1u << (i & 31);
        k[0] -= 1;
      } else {  // digit -1: k += 1
        d.neg[i >> 5] |= 1u << (i & 31);
        for (int q = 0; q < 5 && ++k[q] == 0; q++) {
        }
      }
      d.top = i;
    }
    for (int q = 0; q < 4; q++) k[q] = (k[q] >> 1) | (k[q + 1] << 63);
    k[4] >>= 1;
  }
  ArenaScope scope(c.arena);
  G1Xyzz* sums = c.arena.alloc_n<G1Xyzz>(n);
  hipLaunchKernelGGL(g1_axpy_kernel, dim3(blocks_for(n, 128, 1 << 16)), dim3(128), 0, c.stream, a, b, n, d, sums);
  hipLaunchKernelGGL(g1_normalize_kernel, dim3(blocks_for((n + AX_BATCH - 1) / AX_BATCH, 128, 1 << 16)), dim3(128), 0, c.stream,
                     (const G1Xyzz*)sums, n, out);
}

// ------------------------------------------------------------------ the field side of a round
__global__ void ipa_cross_kernel(const Fr* __restrict__ coeffs, const Fr* __restrict__ zs, size_t mid, Fr* __restrict__ partials) {
  __shared__ Fr lds[4];
  Fr cl = Fr::zero(), cr = Fr::zero();
  GSTRIDE(i, mid) {
    cl = add(cl, mul(coeffs[mid + i], zs[i]));
    cr = add(cr, mul(coeffs[i], zs[mid + i]));
  }
  cl = block_reduce_sum(cl, lds);
  cr = block_reduce_sum(cr, lds);
  if (threadIdx.x == 0) partials[2 * blockIdx.x] = cl, partials[2 * blockIdx.x + 1] = cr;
}
__global__ void ipa_cross_finish_kernel(const Fr* __restrict__ partials, int blocks, Fr* __restrict__ out) {
  __shared__ Fr lds[4];
  Fr cl = Fr::zero(), cr = Fr::zero();
  for (int i = threadIdx.x; i < blocks; i += blockDim.x) cl = add(cl, partials[2 * i]), cr = add(cr, partials[2 * i + 1]);
  cl = block_reduce_sum(cl, lds);
  cr = block_reduce_sum(cr, lds);
  if (threadIdx.x == 0) out[0] = cl, out[1] = cr;
}

void k_ipa_cross(Ctx& c, const Fr* coeffs, const Fr* zs, size_t mid, Fr* d_partials, Fr* d_out) {
  ProfScope ps(c, "ipa_cross", 128.0 * mid, 2.0 * mid, (double)mid);
  const unsigned blocks = blocks_for(mid, 256, IPA_CROSS_BLOCKS);
  hipLaunchKernelGGL(ipa_cross_kernel, dim3(blocks), dim3(256), 0, c.stream, coeffs, zs, mid, d_partials);
  hipLaunchKernelGGL(ipa_cross_finish_kernel, dim3(1), dim3(256), 0, c.stream, (const Fr*)d_partials, (int)blocks, d_out);
}

// (no __restrict__: from the second round on the fold is in place, out_c == coeffs and out_z == zs; entry i is read and
// written by the same thread and the upper halves are only read)
__global__ void ipa_fold_fr_kernel(const Fr* coeffs, const Fr* zs, size_t mid, Fr xi_inv, Fr xi, Fr* out_c, Fr* out_z) {
  GSTRIDE(i, mid) {
    const Fr cv = add(coeffs[i], mul(xi_inv, coeffs[mid + i])), zv = add(zs[i], mul(xi, zs[mid + i]));
    out_c[i] = cv, out_z[i] = zv;
  }
}

void k_ipa_fold_fr(Ctx& c, const Fr* coeffs, const Fr* zs, size_t mid, const Fr& xi_inv, const Fr& xi, Fr* out_c, Fr* out_z) {
  ProfScope ps(c, "ipa_fold_fr", 192.0 * mid, 2.0 * mid, (double)mid);
  hipLaunchKernelGGL(ipa_fold_fr_kernel, dim3(blocks_for(mid, 256, 4096)), dim3(256), 0, c.stream, coeffs, zs, mid, xi_inv, xi,
                     out_c, out_z);
}

// ------------------------------------------------------------------ Hyrax: the combined row
// slice y sums the rows y, y + S, ..: adjacent threads read adjacent columns of a row (coalesced), every row is read once
__global__ void hyrax_combine_kernel(const Fr* __restrict__ poly, const Fr* __restrict__ w, size_t rows, size_t row_len,
                                     Fr* __restrict__ partial) {
  GSTRIDE(c, row_len) {
    Fr acc = Fr::zero();
    for (size_t r = blockIdx.y; r < rows; r += gridDim.y) acc = add(acc, mul(w[r], poly[r * row_len + c]));
    partial[(size_t)blockIdx.y * row_len + c] = acc;
  }
}
__global__ void hyrax_combine_sum_kernel(const Fr* __restrict__ partial, size_t slices, size_t row_len, Fr* __restrict__ out) {
  GSTRIDE(c, row_len) {
    Fr acc = partial[c];
    for (size_t s = 1; s < slices; s++) acc = add(acc, partial[s * row_len + c]);
    out[c] = acc;
  }
}

void k_hyrax_combine(Ctx& c, const Fr* poly, const Fr* w, size_t rows, size_t row_len, Fr* out) {
  ProfScope ps(c, "hyrax_combine", 32.0 * rows * row_len, 1.0 * rows * row_len, (double)(rows * row_len));
  const size_t slices = std::min<size_t>(rows, 64);
  ArenaScope scope(c.arena);
  Fr* partial = slices > 1 ? c.arena.alloc_n<Fr>(slices * row_len) : out;
  hipLaunchKernelGGL(hyrax_combine_kernel, dim3(blocks_for(row_len, 256, 4096), (unsigned)slices), dim3(256), 0, c.stream, poly, w,
                     rows, row_len, partial);
  if (slices > 1)
    hipLaunchKernelGGL(hyrax_combine_sum_kernel, dim3(blocks_for(row_len, 256, 4096)), dim3(256), 0, c.stream,
                       (const Fr*)partial, slices, row_len, out);
}

}  // namespace lh
