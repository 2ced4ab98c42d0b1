// Test-only probe of the device field and curve primitives (ff.cuh, wide.cuh, ec.cuh): tests/field_edges.py drives it
// through ctypes.  Built as libff_probe.so next to liblasso_hip.so; not part of the library or its C ABI.
//
// ffp_run(op, field, k, in, in_stride, out, out_stride, n): n cases, case i reads in[i * in_stride ..] and writes
// out[i * out_stride ..] (u32 words).  One thread handles one case; the quad-cooperative routines take the 4 lanes of a
// quad per case and write all four lanes' results.  Host buffers: copy in, one launch, copy out.  Returns the HIP status
// (0 = success), or -8 for arguments the op cannot take; it never aborts.
// ffp_run_host: the same ops through the host forms of the headers (mul_scan / dot_scan / dot_scan_cols run as the
// host's mul / dot); the device-only ones (Wide, add_mixed_lazy, the quad routines) answer -9.
//
// Field elements are 8 stored limbs (Montgomery form, as in memory).  Per-op layouts (words):
//   unary ops (NEG DBL SQR CANON TO_MONT FROM_MONT INV): a[8] -> r[8];  IS_ZERO_LAZY: a[8] -> {0, 1}
//   binary ops (ADD SUB MUL MUL_SCAN MUL_LAZY ADD_LAZY SUB_LAZY): a[8] b[8] -> r[8];  POW: a[8] e[8] -> a^e [8]
//   FROM_U64: lo, hi -> r[8];  DOT_SCAN / DOT_COLS: a[0..k)[8] b[0..k)[8] -> r[8]
//   WIDE (Fr): start[10] t {w[8] v}[t] -> raw[10] wide_reduce[8] wide_redc[8]
//   curves (Fq; an XYZZ point is x y zz zzz [32], an affine point x y [16]):
//     DBL_AFFINE: q[16] -> [32]   DBL: p[32] -> [32]   ADD: p[32] q[32] -> [32]
//     ADD_MIXED: p[32] q[16] negate -> [32]   ADD_MIXED_LAZY: p[32] q[16] negate -> lazy [32], canon_xyzz [32]
//     DBL_QUAD: p[32] -> 4 lanes x [32]       ADD_QUAD: p[32] q[32] -> 4 lanes x [32]
#include <hip/hip_runtime.h>
#include "ec.cuh"
#include "ff.cuh"
#include "wide.cuh"

namespace lh {
namespace probe {

enum Op {
  ADD = 0, SUB, NEG, DBL, MUL, MUL_SCAN, SQR, DOT_SCAN, DOT_COLS, MUL_LAZY, ADD_LAZY, SUB_LAZY, CANON, IS_ZERO_LAZY,
  TO_MONT, FROM_MONT, FROM_U64, INV, POW, WIDE, EC_DBL_AFFINE, EC_DBL, EC_ADD_MIXED, EC_ADD_MIXED_LAZY, EC_ADD,
  EC_DBL_QUAD, EC_ADD_QUAD, NUM_OPS
};
constexpr int ERR_ARG = -8, ERR_HOST = -9, MAX_CASES = 1 << 16, MAX_WIDE_TERMS = 64;

// words a case reads / writes (WIDE: without its terms)
static int in_words(int op, int k) {
  switch (op) {
    case NEG: case DBL: case SQR: case CANON: case IS_ZERO_LAZY: case TO_MONT: case FROM_MONT: case INV: return 8;
    case FROM_U64: return 2;
    case DOT_SCAN: case DOT_COLS: return 16 * k;
    case WIDE: return 11;
    case EC_DBL_AFFINE: return 16;
    case EC_DBL: case EC_DBL_QUAD: return 32;
    case EC_ADD_MIXED: case EC_ADD_MIXED_LAZY: return 49;
    case EC_ADD: case EC_ADD_QUAD: return 64;
    default: return 16;
  }
}
static int out_words(int op) {
  switch (op) {
    case IS_ZERO_LAZY: return 1;
    case WIDE: return 26;
    case EC_DBL_AFFINE: case EC_DBL: case EC_ADD_MIXED: case EC_ADD: return 32;
    case EC_ADD_MIXED_LAZY: return 64;
    case EC_DBL_QUAD: case EC_ADD_QUAD: return 128;
    default: return 8;
  }
}

template <class P>
LH_HD Fp<P> ld(const uint32_t* s) {
  Fp<P> r;
  for (int i = 0; i < 8; i++) r.l[i] = s[i];
  return r;
}
template <class P>
LH_HD void st(uint32_t* d, const Fp<P>& a) {
  for (int i = 0; i < 8; i++) d[i] = a.l[i];
}
LH_HD G1Affine ld_aff(const uint32_t* s) {
  G1Affine r;
  r.x = ld<FqParams>(s), r.y = ld<FqParams>(s + 8);
  return r;
}
LH_HD G1Xyzz ld_xyzz(const uint32_t* s) {
  G1Xyzz r;
  r.x = ld<FqParams>(s), r.y = ld<FqParams>(s + 8), r.zz = ld<FqParams>(s + 16), r.zzz = ld<FqParams>(s + 24);
  return r;
}
LH_HD void st_xyzz(uint32_t* d, const G1Xyzz& p) {
  st(d, p.x), st(d + 8, p.y), st(d + 16, p.zz), st(d + 24, p.zzz);
}

// one case of a per-thread op (the quad routines are below); K is the dot length, 0 elsewhere
template <class P, int OP, int K>
LH_HD void eval(const uint32_t* in, uint32_t* out) {
  typedef Fp<P> F;
  if constexpr (OP == NEG) st(out, neg(ld<P>(in)));
  else if constexpr (OP == DBL) st(out, dbl(ld<P>(in)));
  else if constexpr (OP == SQR) st(out, sqr(ld<P>(in)));
  else if constexpr (OP == CANON) st(out, canon(ld<P>(in)));
  else if constexpr (OP == IS_ZERO_LAZY) out[0] = is_zero_lazy(ld<P>(in)) ? 1u : 0u;
  else if constexpr (OP == TO_MONT) st(out, to_mont(ld<P>(in)));
  else if constexpr (OP == FROM_MONT) st(out, from_mont(ld<P>(in)));
  else if constexpr (OP == INV) st(out, inv(ld<P>(in)));
  else if constexpr (OP == FROM_U64) st(out, from_u64<P>((uint64_t)in[0] | ((uint64_t)in[1] << 32)));
  else if constexpr (OP == ADD) st(out, add(ld<P>(in), ld<P>(in + 8)));
  else if constexpr (OP == SUB) st(out, sub(ld<P>(in), ld<P>(in + 8)));
  else if constexpr (OP == MUL) st(out, mul(ld<P>(in), ld<P>(in + 8)));
  else if constexpr (OP == MUL_LAZY) st(out, mul_lazy(ld<P>(in), ld<P>(in + 8)));
  else if constexpr (OP == ADD_LAZY) st(out, add_lazy(ld<P>(in), ld<P>(in + 8)));
  else if constexpr (OP == SUB_LAZY) st(out, sub_lazy(ld<P>(in), ld<P>(in + 8)));
  else if constexpr (OP == POW) {
    uint32_t e[8];
    for (int i = 0; i < 8; i++) e[i] = in[8 + i];
    st(out, pow_limbs(ld<P>(in), e));
  } else if constexpr (OP == MUL_SCAN) {
#if defined(__HIP_DEVICE_COMPILE__)
    st(out, mul_scan(ld<P>(in), ld<P>(in + 8)));
#else
    st(out, mul(ld<P>(in), ld<P>(in + 8)));
#endif
  } else if constexpr (OP == DOT_SCAN || OP == DOT_COLS) {
    F a[K], b[K];
    for (int j = 0; j < K; j++) a[j] = ld<P>(in + 8 * j), b[j] = ld<P>(in + 8 * (K + j));
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (OP == DOT_SCAN) st(out, dot_scan<P, K>(a, b));
    else st(out, dot_scan_cols<P, K>(a, b));
#else
    st(out, dot<P, K>(a, b));
#endif
  } else if constexpr (OP == EC_DBL_AFFINE) st_xyzz(out, dbl_affine(ld_aff(in)));
  else if constexpr (OP == EC_DBL) st_xyzz(out, dbl(ld_xyzz(in)));
  else if constexpr (OP == EC_ADD) st_xyzz(out, add(ld_xyzz(in), ld_xyzz(in + 32)));
  else if constexpr (OP == EC_ADD_MIXED) st_xyzz(out, add_mixed(ld_xyzz(in), ld_aff(in + 32), in[48] != 0));
#if defined(__HIP_DEVICE_COMPILE__)
  else if constexpr (OP == EC_ADD_MIXED_LAZY) {
    const G1Xyzz r = add_mixed_lazy(ld_xyzz(in), ld_aff(in + 32), in[48] != 0);
    st_xyzz(out, r), st_xyzz(out + 32, canon_xyzz(r));
  } else if constexpr (OP == WIDE) {
    Wide acc;
    for (int i = 0; i < 10; i++) acc.l[i] = in[i];
    const uint32_t t = in[10];
    for (uint32_t j = 0; j < t; j++) wide_mac(acc, ld<FrParams>(in + 11 + 9 * j), in[11 + 9 * j + 8]);
    for (int i = 0; i < 10; i++) out[i] = acc.l[i];
    st(out + 10, wide_reduce(acc));
    st(out + 18, wide_redc(acc));
  }
#endif
}

template <class P, int OP, int K>
__global__ void probe_kernel(const uint32_t* __restrict__ in, int in_stride, uint32_t* __restrict__ out, int out_stride,
                             int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) eval<P, OP, K>(in + (size_t)i * in_stride, out + (size_t)i * out_stride);
}

// lanes 4i..4i+3 take case i with the same operands; lane l writes its result to out[i * out_stride + 32 l ..]
template <int OP>
__global__ void probe_quad_kernel(const uint32_t* __restrict__ in, int in_stride, uint32_t* __restrict__ out,
                                  int out_stride, int n) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x, i = t >> 2;
  if (i >= n) return;  // (whole quads: the case decides, not the lane)
  const uint32_t* c = in + (size_t)i * in_stride;
  G1Xyzz r;
  if constexpr (OP == EC_DBL_QUAD) r = dbl_quad(ld_xyzz(c));
  else r = add_quad(ld_xyzz(c), ld_xyzz(c + 32));
  st_xyzz(out + (size_t)i * out_stride + 32 * (t & 3), r);
}

struct Job {
  const uint32_t* in;
  int in_stride;
  uint32_t* out;
  int out_stride;
  int n;
};

template <class P, int OP, int K>
int run_dev(const Job& j) {
  const size_t in_bytes = (size_t)j.n * j.in_stride * 4, out_bytes = (size_t)j.n * j.out_stride * 4;
  uint32_t *din = nullptr, *dout = nullptr;
  hipError_t e = hipMalloc(&din, in_bytes ? in_bytes : 4);
  if (e == hipSuccess) e = hipMalloc(&dout, out_bytes ? out_bytes : 4);
  if (e == hipSuccess) e = hipMemcpy(din, j.in, in_bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(dout, 0, out_bytes);
  if (e == hipSuccess) {
    const int lanes = OP == EC_DBL_QUAD || OP == EC_ADD_QUAD ? 4 : 1, threads = j.n * lanes;
    const dim3 grid((unsigned)((threads + 255) / 256));
    if constexpr (OP == EC_DBL_QUAD || OP == EC_ADD_QUAD)
      hipLaunchKernelGGL(probe_quad_kernel<OP>, grid, 256, 0, 0, din, j.in_stride, dout, j.out_stride, j.n);
    else
      hipLaunchKernelGGL((probe_kernel<P, OP, K>), grid, 256, 0, 0, din, j.in_stride, dout, j.out_stride, j.n);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(j.out, dout, out_bytes, hipMemcpyDeviceToHost);
  if (din) (void)hipFree(din);
  if (dout) (void)hipFree(dout);
  return (int)e;
}

template <class P, int OP, int K>
int run_host(const Job& j) {
  if constexpr (OP == WIDE || OP == EC_ADD_MIXED_LAZY || OP == EC_DBL_QUAD || OP == EC_ADD_QUAD) {
    return ERR_HOST;
  } else {
    for (int i = 0; i < j.n; i++) eval<P, OP, K>(j.in + (size_t)i * j.in_stride, j.out + (size_t)i * j.out_stride);
    return 0;
  }
}

template <bool DEV, class P, int OP, int K>
int run(const Job& j) {
  return DEV ? run_dev<P, OP, K>(j) : run_host<P, OP, K>(j);
}

template <bool DEV, class P, int OP>
int run_dot(int k, const Job& j) {
  switch (k) {
    case 1: return run<DEV, P, OP, 1>(j);
    case 2: return run<DEV, P, OP, 2>(j);
    case 3: return run<DEV, P, OP, 3>(j);
    case 4: return run<DEV, P, OP, 4>(j);
    case 5: return run<DEV, P, OP, 5>(j);
    case 6: return run<DEV, P, OP, 6>(j);
    case 7: return run<DEV, P, OP, 7>(j);
    case 8: return run<DEV, P, OP, 8>(j);
    case 10: return run<DEV, P, OP, 10>(j);
    case 11: return run<DEV, P, OP, 11>(j);
    case 15: return run<DEV, P, OP, 15>(j);
    case 16: return run<DEV, P, OP, 16>(j);
    default: return ERR_ARG;
  }
}

template <bool DEV, class P>
int run_field(int op, int k, const Job& j) {
  switch (op) {
    case ADD: return run<DEV, P, ADD, 0>(j);
    case SUB: return run<DEV, P, SUB, 0>(j);
    case NEG: return run<DEV, P, NEG, 0>(j);
    case DBL: return run<DEV, P, DBL, 0>(j);
    case MUL: return run<DEV, P, MUL, 0>(j);
    case MUL_SCAN: return run<DEV, P, MUL_SCAN, 0>(j);
    case SQR: return run<DEV, P, SQR, 0>(j);
    case DOT_SCAN: return run_dot<DEV, P, DOT_SCAN>(k, j);
    case DOT_COLS: return run_dot<DEV, P, DOT_COLS>(k, j);
    case MUL_LAZY: return run<DEV, P, MUL_LAZY, 0>(j);
    case ADD_LAZY: return run<DEV, P, ADD_LAZY, 0>(j);
    case SUB_LAZY: return run<DEV, P, SUB_LAZY, 0>(j);
    case CANON: return run<DEV, P, CANON, 0>(j);
    case IS_ZERO_LAZY: return run<DEV, P, IS_ZERO_LAZY, 0>(j);
    case TO_MONT: return run<DEV, P, TO_MONT, 0>(j);
    case FROM_MONT: return run<DEV, P, FROM_MONT, 0>(j);
    case FROM_U64: return run<DEV, P, FROM_U64, 0>(j);
    case INV: return run<DEV, P, INV, 0>(j);
    case POW: return run<DEV, P, POW, 0>(j);
    default: return ERR_ARG;
  }
}

template <bool DEV>
int dispatch(int op, int field, int k, const uint32_t* in, int in_stride, uint32_t* out, int out_stride, int n) {
  if (op < 0 || op >= NUM_OPS || field < 0 || field > 1 || n < 0 || n > MAX_CASES || !in || !out) return ERR_ARG;
  if ((op == DOT_SCAN || op == DOT_COLS) != (k != 0)) return ERR_ARG;
  if (in_stride < in_words(op, k) || out_stride < out_words(op)) return ERR_ARG;
  if (op == WIDE) {  // Fr only; every case's terms must lie inside its stride
    if (field != 0) return ERR_ARG;
    for (int i = 0; i < n; i++) {
      const uint32_t t = in[(size_t)i * in_stride + 10];
      if (t > MAX_WIDE_TERMS || 11 + 9 * (int)t > in_stride) return ERR_ARG;
    }
    return run<DEV, FrParams, WIDE, 0>({in, in_stride, out, out_stride, n});
  }
  const Job j{in, in_stride, out, out_stride, n};
  if (op >= EC_DBL_AFFINE) {  // the curve is over Fq
    if (field != 1) return ERR_ARG;
    switch (op) {
      case EC_DBL_AFFINE: return run<DEV, FqParams, EC_DBL_AFFINE, 0>(j);
      case EC_DBL: return run<DEV, FqParams, EC_DBL, 0>(j);
      case EC_ADD_MIXED: return run<DEV, FqParams, EC_ADD_MIXED, 0>(j);
      case EC_ADD_MIXED_LAZY: return run<DEV, FqParams, EC_ADD_MIXED_LAZY, 0>(j);
      case EC_ADD: return run<DEV, FqParams, EC_ADD, 0>(j);
      case EC_DBL_QUAD: return run<DEV, FqParams, EC_DBL_QUAD, 0>(j);
      default: return run<DEV, FqParams, EC_ADD_QUAD, 0>(j);
    }
  }
  return field == 0 ? run_field<DEV, FrParams>(op, k, j) : run_field<DEV, FqParams>(op, k, j);
}

}  // namespace probe
}  // namespace lh

extern "C" {
// field: 0 = Fr, 1 = Fq; k: the dot length for DOT_SCAN / DOT_COLS, 0 for every other op
int ffp_run(int op, int field, int k, const uint32_t* in, int in_stride, uint32_t* out, int out_stride, int n) {
  return lh::probe::dispatch<true>(op, field, k, in, in_stride, out, out_stride, n);
}
int ffp_run_host(int op, int field, int k, const uint32_t* in, int in_stride, uint32_t* out, int out_stride, int n) {
  return lh::probe::dispatch<false>(op, field, k, in, in_stride, out, out_stride, n);
}
}
