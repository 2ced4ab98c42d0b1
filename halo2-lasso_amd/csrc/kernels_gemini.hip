// Kernels of the Gemini opening and of the batched univariate KZG opening under it (reference
// pcs/multilinear/gemini.rs:78-138, pcs/univariate/kzg.rs:301-354).  Everything between the three large
// MSMs of an opening, batched over the polys of one opening so that the launch count does not grow with num_vars:
//   fold tail      every fold fs[i] from the level of GM_TAIL_IN coefficients down, inside one workgroup's LDS (the levels
//                  above it stream through k_fix_var, one launch each)
//   eval_even_odd  E_s = sum_j f[2j] x2^j and O_s = sum_j f[2j+1] x2^j of every segment s in one pass over its
//                  coefficients: f(p) = E(p^2) + p O(p^2), so fs[0](beta) and fs[0](-beta) share one pass
//   suffix Horner  out[i] = f[i] + x out[i + stride], batched over segments of different lengths: out[stride..] is the
//                  quotient by X^stride - x (stride 1: X - p; stride 2: (X - p)(X + p) with x = p^2), three launches
//   combine        out[j] = sum_{k : j < len_k} w_k p_k[j] over vectors of different lengths, every output written once
#include <hip/hip_runtime.h>
#include <algorithm>
#include "dev.hpp"
#include "launch.cuh"
#include "reduce.cuh"

namespace lh {

static inline unsigned blocks_for(size_t n, size_t block = 256, size_t cap = 4096) {
  size_t g = (n + block - 1) / block;
  return (unsigned)(g < 1 ? 1 : g > cap ? cap : g);
}

__device__ __forceinline__ Fr pow_u64(Fr base, uint64_t e) {
  Fr acc = Fr::one();
  for (; e; e >>= 1) {
    if (e & 1) acc = mul(acc, base);
    base = mul(base, base);
  }
  return acc;
}

// ------------------------------------------------------------------ fold chain
struct GmFoldXs {
  Fr x[GM_MAX_VARS];
};
// in: 2^in_log coefficients (<= GM_TAIL_IN); level k = 0 .. levels - 1 binds with xs.x[k] and lands at out + off_k,
// off_0 = 0, off_{k+1} = off_k + 2^(in_log - 1 - k): the arena layout of the folds
__global__ void __launch_bounds__(256) gm_fold_tail_kernel(const Fr* __restrict__ in, int in_log, int levels, GmFoldXs xs,
                                                             Fr* __restrict__ out) {
  __shared__ Fr a[GM_TAIL_IN], b[GM_TAIL_IN / 2];
  const size_t n_in = (size_t)1 << in_log;
  for (size_t i = threadIdx.x; i < n_in; i += blockDim.x) a[i] = in[i];
  __syncthreads();
  Fr *src = a, *dst = b;
  size_t off = 0;
  for (int k = 0; k < levels; k++) {
    const size_t n_out = n_in >> (k + 1);
    const Fr x = xs.x[k];
    for (size_t j = threadIdx.x; j < n_out; j += blockDim.x) {
      const Fr e0 = src[2 * j], e1 = src[2 * j + 1];
      const Fr v = add(mul(sub(e1, e0), x), e0);
      dst[j] = v;
      out[off + j] = v;
    }
    off += n_out;
    __syncthreads();
    Fr* t = src;
    src = dst, dst = t;  // (the next level writes n_out / 2 entries: they fit either buffer)
  }
}

void k_gm_fold_chain(Ctx& c, const Fr* poly, size_t num_vars, const Fr* xs, Fr* folds) {
  LH_REQUIRE(num_vars >= 1 && num_vars <= (size_t)GM_MAX_VARS, LH_ERR_ARG, "gemini folds: bad num_vars");
  const Fr* src = poly;
  size_t len = (size_t)1 << num_vars, off = 0, level = 1;  // `level`: the fold being made, from src (len coefficients)
  for (; level < num_vars && len > GM_TAIL_IN; level++) {
    k_fix_var(c, src, len, xs[level - 1], folds + off);
    src = folds + off;
    off += len >> 1;
    len >>= 1;
  }
  if (level >= num_vars) return;
  GmFoldXs p;
  const int levels = (int)(num_vars - level);
  for (int k = 0; k < levels; k++) p.x[k] = xs[level - 1 + k];
  int in_log = 0;
  while (((size_t)1 << in_log) < len) in_log++;
  ProfScope ps(c, "gm_fold_tail", 64.0 * len, (double)len, (double)len);
  hipLaunchKernelGGL(gm_fold_tail_kernel, 1, 256, 0, c.stream, src, in_log, levels, p, folds + off);
}

// ------------------------------------------------------------------ E(x2), O(x2) of every segment
constexpr int GM_SEGS_PER_LAUNCH = 32;
constexpr unsigned GM_EVAL_MAX_BLOCKS = 1024;
struct GmEvalDev {
  const Fr* f;
  uint64_t pairs;
  Fr x2, xT;  // xT = x2^(nblocks * 256): a thread walks its pairs g, g + T, g + 2T, .. by Horner in xT
  uint32_t nblocks;
};
struct GmEvalPack {
  GmEvalDev s[GM_SEGS_PER_LAUNCH];
};
// partial[(seg * gridDim.x + block) * 2 + {0, 1}] = this block's share of E, O (zero for the blocks a short segment leaves idle)
__global__ void __launch_bounds__(256) gm_eval_kernel(GmEvalPack p, Fr* __restrict__ partial) {
  __shared__ Fr lds[4];
  const GmEvalDev& s = p.s[blockIdx.y];
  Fr e = Fr::zero(), o = Fr::zero();
  const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (blockIdx.x < s.nblocks && g < s.pairs) {
    const uint64_t T = (uint64_t)s.nblocks * 256;
    const Fr xT = s.xT;
    for (uint64_t k = (s.pairs - 1 - g) / T + 1; k-- > 0;) {
      const uint64_t idx = g + k * T;
      e = add(mul(e, xT), s.f[2 * idx]);
      o = add(mul(o, xT), s.f[2 * idx + 1]);
    }
    const Fr w = pow_u64(s.x2, g);
    e = mul(e, w), o = mul(o, w);
  }
  e = block_reduce_sum(e, lds);
  o = block_reduce_sum(o, lds);
  if (threadIdx.x == 0) {
    Fr* dst = partial + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 2;
    dst[0] = e, dst[1] = o;
  }
}
// out[2 seg + {0, 1}] = sum over the blocks
__global__ void __launch_bounds__(256) gm_eval_sum_kernel(const Fr* __restrict__ partial, unsigned nblocks, Fr* __restrict__ out) {
  __shared__ Fr lds[4];
  const Fr* src = partial + (size_t)blockIdx.x * nblocks * 2;
  Fr e = Fr::zero(), o = Fr::zero();
  for (unsigned b = threadIdx.x; b < nblocks; b += blockDim.x) e = add(e, src[2 * b]), o = add(o, src[2 * b + 1]);
  e = block_reduce_sum(e, lds);
  o = block_reduce_sum(o, lds);
  if (threadIdx.x == 0) out[2 * blockIdx.x] = e, out[2 * blockIdx.x + 1] = o;
}

void k_gm_eval_even_odd(Ctx& c, const GmEvalSeg* segs, size_t count, Fr* out) {
  if (!count) return;
  ArenaScope scope(c.arena);
  Fr* d_out = c.arena.alloc_n<Fr>(2 * count);
  double total = 0;
  for (size_t base = 0; base < count; base += GM_SEGS_PER_LAUNCH) {
    const size_t k = std::min<size_t>(count - base, GM_SEGS_PER_LAUNCH);
    GmEvalPack p;
    unsigned gx = 1;
    for (size_t i = 0; i < k; i++) {
      const GmEvalSeg& s = segs[base + i];
      LH_REQUIRE(s.len >= 2 && s.len % 2 == 0, LH_ERR_ARG, "even/odd evaluation: odd length");
      GmEvalDev& d = p.s[i];
      d.f = s.f, d.pairs = s.len / 2, d.x2 = s.x2;
      d.nblocks = blocks_for(d.pairs, 256, GM_EVAL_MAX_BLOCKS);
      gx = std::max(gx, d.nblocks);
      Fr xT = Fr::one(), sq = s.x2;  // ff.cuh arithmetic is host-callable
      for (uint64_t e = (uint64_t)d.nblocks * 256; e; e >>= 1) {
        if (e & 1) xT = mul(xT, sq);
        sq = mul(sq, sq);
      }
      d.xT = xT;
      total += (double)s.len;
    }
    Fr* partial = c.arena.alloc_n<Fr>((size_t)k * gx * 2);
    {
      ProfScope ps(c, "gm_eval_even_odd", 32.0 * total, total, total);
      hipLaunchKernelGGL(gm_eval_kernel, dim3(gx, (unsigned)k), 256, 0, c.stream, p, partial);
    }
    ProfScope ps(c, "gm_eval_sum", 64.0 * k * gx, 0.0, (double)k * gx);
    hipLaunchKernelGGL(gm_eval_sum_kernel, (unsigned)k, 256, 0, c.stream, partial, gx, d_out + 2 * base);
  }
  c.d2h(out, d_out, 2 * count * sizeof(Fr));
}

// ------------------------------------------------------------------ out[i] = f[i] + x out[i + stride], batched
// A segment of stride s is s interleaved recurrences ("lanes"); every lane is cut into chunks of GM_CHUNK positions.
//   values   L[c * s + lane] = the chunk as a polynomial in x
//   scan     T_c = L_c + x^GM_CHUNK T_{c+1} per (segment, lane), one workgroup each, in place
//   expand   the recurrence inside every chunk, seeded with T_{c+1}
struct GmHornerDev {
  const Fr* f;
  Fr* out;
  uint64_t len;
  Fr x, y;  // y = x^GM_CHUNK
  uint32_t stride, loff;  // loff: where this segment's chunk values start
};
struct GmHornerPack {
  GmHornerDev s[GM_SEGS_PER_LAUNCH];
};
__device__ __forceinline__ uint64_t gm_lane_positions(uint64_t len, uint32_t stride, uint32_t lane) {
  return len > lane ? (len - lane + stride - 1) / stride : 0;
}
__global__ void gm_horner_values_kernel(GmHornerPack p, Fr* __restrict__ L) {
  const GmHornerDev& s = p.s[blockIdx.y];
  const uint64_t chunks0 = (gm_lane_positions(s.len, s.stride, 0) + GM_CHUNK - 1) / GM_CHUNK;
  GSTRIDE(u, chunks0 * s.stride) {
    const uint32_t lane = (uint32_t)(u % s.stride);
    const uint64_t ch = u / s.stride, pos = gm_lane_positions(s.len, s.stride, lane);
    const uint64_t start = ch * GM_CHUNK, end = start + GM_CHUNK < pos ? start + GM_CHUNK : pos;
    Fr acc = Fr::zero();
    for (uint64_t i = end; i-- > start;) acc = add(mul(acc, s.x), s.f[i * s.stride + lane]);  // (start >= end: an empty chunk)
    L[s.loff + u] = acc;
  }
}
__global__ void __launch_bounds__(256) gm_horner_scan_kernel(GmHornerPack p, Fr* __restrict__ L) {
  __shared__ Fr v[256];
  __shared__ Fr yK_s;
  const GmHornerDev& s = p.s[blockIdx.x];
  const uint32_t lane = blockIdx.y;
  if (lane >= s.stride) return;
  const uint64_t M = (gm_lane_positions(s.len, s.stride, 0) + GM_CHUNK - 1) / GM_CHUNK;  // (lane 0's count: empty chunks hold zero)
  if (!M) return;
  Fr* Ls = L + s.loff + lane;
  const uint64_t K = (M + 255) / 256, t = threadIdx.x;
  const uint64_t lo = t * K < M ? t * K : M, hi = (t + 1) * K < M ? (t + 1) * K : M;
  Fr acc = Fr::zero();
  for (uint64_t ch = hi; ch-- > lo;) acc = add(mul(acc, s.y), Ls[ch * s.stride]);
  v[t] = acc;
  if (t == 0) yK_s = pow_u64(s.y, K);
  __syncthreads();
  if (t == 0) {  // carries: v[t] <- T at the end of thread t's range
    const Fr yK = yK_s;
    Fr carry = Fr::zero();
    for (int i = 255; i >= 0; i--) {
      const Fr own = v[i];
      v[i] = carry;
      carry = add(mul(carry, yK), own);
    }
  }
  __syncthreads();
  acc = v[t];
  for (uint64_t ch = hi; ch-- > lo;) {
    acc = add(mul(acc, s.y), Ls[ch * s.stride]);
    Ls[ch * s.stride] = acc;
  }
}
__global__ void gm_horner_expand_kernel(GmHornerPack p, const Fr* __restrict__ T) {
  const GmHornerDev& s = p.s[blockIdx.y];
  const uint64_t chunks0 = (gm_lane_positions(s.len, s.stride, 0) + GM_CHUNK - 1) / GM_CHUNK;
  GSTRIDE(u, chunks0 * s.stride) {
    const uint32_t lane = (uint32_t)(u % s.stride);
    const uint64_t ch = u / s.stride, pos = gm_lane_positions(s.len, s.stride, lane);
    const uint64_t start = ch * GM_CHUNK, end = start + GM_CHUNK < pos ? start + GM_CHUNK : pos;
    Fr acc = ch + 1 < chunks0 ? T[s.loff + u + s.stride] : Fr::zero();
    for (uint64_t i = end; i-- > start;) {
      acc = add(mul(acc, s.x), s.f[i * s.stride + lane]);
      s.out[i * s.stride + lane] = acc;
    }
  }
}

void k_gm_suffix_horner(Ctx& c, const GmHornerSeg* segs, size_t count) {
  for (size_t base = 0; base < count; base += GM_SEGS_PER_LAUNCH) {
    const size_t k = std::min<size_t>(count - base, GM_SEGS_PER_LAUNCH);
    ArenaScope scope(c.arena);
    GmHornerPack p;
    size_t lsize = 0, max_units = 1;
    uint32_t max_stride = 1;
    double total = 0;
    for (size_t i = 0; i < k; i++) {
      const GmHornerSeg& s = segs[base + i];
      LH_REQUIRE(s.stride >= 1 && s.stride <= GM_MAX_STRIDE && s.len >= 1, LH_ERR_ARG, "suffix Horner: bad segment");
      GmHornerDev& d = p.s[i];
      d.f = s.f, d.out = s.out, d.len = s.len, d.x = s.x, d.stride = s.stride;
      Fr y = s.x;
      for (size_t e = 1; e < GM_CHUNK; e <<= 1) y = mul(y, y);
      d.y = y;
      const size_t pos0 = (s.len + s.stride - 1) / s.stride, units = (pos0 + GM_CHUNK - 1) / GM_CHUNK * s.stride;
      LH_REQUIRE(lsize + units < ((size_t)1 << 32), LH_ERR_ARG, "suffix Horner: batch too large");
      d.loff = (uint32_t)lsize;
      lsize += units;
      max_units = std::max(max_units, units);
      max_stride = std::max(max_stride, s.stride);
      total += (double)s.len;
    }
    Fr* L = c.arena.alloc_n<Fr>(lsize);
    {
      ProfScope ps(c, "gm_horner_values", 32.0 * total, total, total);
      hipLaunchKernelGGL(gm_horner_values_kernel, dim3(blocks_for(max_units, 64), (unsigned)k), 64, 0, c.stream, p, L);
    }
    {
      ProfScope ps(c, "gm_horner_scan", 64.0 * lsize, 2.0 * lsize, (double)lsize);
      hipLaunchKernelGGL(gm_horner_scan_kernel, dim3((unsigned)k, max_stride), 256, 0, c.stream, p, L);
    }
    ProfScope ps(c, "gm_horner_expand", 64.0 * total, total, total);
    hipLaunchKernelGGL(gm_horner_expand_kernel, dim3(blocks_for(max_units, 64), (unsigned)k), 64, 0, c.stream, p, L);
  }
}

// ------------------------------------------------------------------ ragged linear combination
struct GmTermDev {
  const Fr* p;
  uint64_t len;
  Fr w;
};
struct GmTermPack {
  GmTermDev t[GM_SEGS_PER_LAUNCH];
};
__global__ void gm_combine_kernel(GmTermPack p, int count, size_t n, int accumulate, Fr* __restrict__ out) {
  GSTRIDE(j, n) {
    Fr acc = accumulate ? out[j] : Fr::zero();
    for (int k = 0; k < count; k++)
      if (j < p.t[k].len) acc = add(acc, mul(p.t[k].w, p.t[k].p[j]));
    out[j] = acc;
  }
}
void k_gm_combine(Ctx& c, const GmTerm* terms, size_t count, size_t n, Fr* out) {
  if (!n) return;
  if (!count) {
    LH_HIP(hipMemsetAsync(out, 0, n * sizeof(Fr), c.stream));
    return;
  }
  for (size_t base = 0; base < count; base += GM_SEGS_PER_LAUNCH) {
    const size_t k = std::min<size_t>(count - base, GM_SEGS_PER_LAUNCH);
    GmTermPack p;
    double total = 0;
    for (size_t i = 0; i < k; i++) {
      p.t[i].p = terms[base + i].p, p.t[i].len = std::min(terms[base + i].len, n), p.t[i].w = terms[base + i].w;
      total += (double)p.t[i].len;
    }
    ProfScope ps(c, "gm_combine", 32.0 * (total + n), total, (double)n);
    hipLaunchKernelGGL(gm_combine_kernel, blocks_for(n), 256, 0, c.stream, p, (int)k, n, base ? 1 : 0, out);
  }
}

}  // namespace lh
