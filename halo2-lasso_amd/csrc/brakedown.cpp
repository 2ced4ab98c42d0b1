// Brakedown PCS, prover half: MultilinearBrakedown<Fr, Keccak256, BrakedownSpec1..6> (reference
// pcs/multilinear/brakedown.rs:89-300) over the expander code of util/code/brakedown.rs.
//   parameters  the spec's formulas in IEEE double (code/brakedown.rs:128-251), row_len by the smallest proof_size;
//   matrices    a seeded sampler of this library's own, in the reference's draw order;
//   commit      every row encoded at once, one launch per cascade stage, then the column leaves and the Merkle tree;
//   open        the combined rows in one pass, then the column openings (paths from a host copy of the tree).
// Restated in tests/brakedown_ref.py, which the tests compare against byte for byte.
#include "brakedown.hpp"
#include <math.h>
#include <algorithm>
#include <map>
#include <memory>

namespace lh {

// ------------------------------------------------------------------ parameters
namespace {
const double LAMBDA = 128.0;
const size_t LOG2_Q = 254;  // bn256::Fr::NUM_BITS
struct Spec {
  double alpha, beta, r;
};
const Spec SPECS[6] = {{0.1195, 0.0284, 1.420}, {0.1380, 0.0444, 1.470}, {0.1780, 0.0610, 1.521},
                       {0.2000, 0.0820, 1.640}, {0.2110, 0.0970, 1.616}, {0.2380, 0.1205, 1.720}};

size_t ceil_(double v) { return v > 0 ? (size_t)ceil(v) : 0; }  // `v.ceil() as usize` saturates at 0
double h(double p) {
  const double q = 1.0 - p;
  return -p * log2(p) - q * log2(q);
}
double mu(const Spec& s) { return s.r - 1.0 - s.r * s.alpha; }
double nu(const Spec& s) { return s.beta + s.alpha * s.beta + 0.03; }
size_t c_n(const Spec& s, size_t n_) {
  const double a = s.alpha, b = s.beta, n = (double)n_;
  return std::min(std::max(ceil_(1.28 * b * n), ceil_(b * n) + 4),
                  ceil_(((110.0 / n) + h(b) + a * h(1.28 * b / a)) / (b * log2(a / (1.28 * b)))));
}
size_t d_n(const Spec& s, size_t log2_q, size_t n_) {
  const double a = s.alpha, b = s.beta, r = s.r, m = mu(s), v = nu(s), n = (double)n_;
  return std::min(ceil_((2.0 * b + ((r - 1.0) + 110.0 / n) / (double)log2_q) * n),
                  ceil_((r * a * h(b / r) + m * h(v / m) + 110.0 / n) / (a * b * log2(m / v))));
}
size_t num_column_opening(const Spec& s) { return ceil_(-LAMBDA / log2(1.0 - (s.beta / s.r) / 3.0)); }

void dimensions(const Spec& s, size_t n, size_t n_0, std::vector<BdDim>& a, std::vector<BdDim>& b) {
  LH_REQUIRE(n > n_0, LH_ERR_ARG, "brakedown: row length must exceed n_0");
  a.clear(), b.clear();
  for (size_t cur = n; cur > n_0;) {
    const size_t nxt = ceil_((double)cur * s.alpha);
    a.push_back(BdDim{cur, nxt, std::min(c_n(s, cur), nxt)});
    cur = nxt;
  }
  for (const BdDim& d : a) {
    const size_t n_prime = ceil_((double)d.m * s.r), total = ceil_((double)d.n * s.r);
    LH_REQUIRE(total >= d.n + n_prime, LH_ERR_ARG, "brakedown: code dimensions underflow (num_vars too small)");
    const size_t m_prime = total - d.n - n_prime;
    b.push_back(BdDim{n_prime, m_prime, std::min(d_n(s, LOG2_Q, d.n), m_prime)});
  }
}
size_t codeword_len(const Spec& s, size_t n, size_t n_0) {
  std::vector<BdDim> a, b;
  dimensions(s, n, n_0, a, b);
  size_t len = a[0].n + b.back().n;
  for (size_t k = 0; k + 1 < a.size(); k++) len += a[k].m;
  for (const BdDim& d : b) len += d.m;
  return len;
}
size_t num_proximity_testing(const Spec& s, size_t n, size_t n_0) {
  return ceil_(LAMBDA / ((double)LOG2_Q - log2((double)codeword_len(s, n, n_0))));
}
size_t proof_size(const Spec& s, size_t n_0, size_t c, size_t r) {
  return (1 + num_proximity_testing(s, c, n_0)) * c + num_column_opening(s) * r;
}
size_t log2_ceil(size_t v) {
  size_t k = 0;
  while (((size_t)1 << k) < v) k++;
  return k;
}

// ------------------------------------------------------------------ the sampler
struct WordStream {
  uint8_t seed[32];
  uint64_t block = 0;
  uint64_t words[4];
  int pos = 4;
  uint64_t next() {
    if (pos == 4) {
      uint8_t msg[40], out[32];
      memcpy(msg, seed, 32);
      for (int i = 0; i < 8; i++) msg[32 + i] = (uint8_t)(block >> (8 * i));
      block++;
      Keccak256 k;
      k.update(msg, 40);
      k.finalize_reset(out);
      memcpy(words, out, 32);
      pos = 0;
    }
    return words[pos++];
  }
  uint64_t uniform(uint64_t m) {
    const unsigned __int128 limit = (((unsigned __int128)1) << 64) / m * m;
    for (;;) {
      const uint64_t w = next();
      if ((unsigned __int128)w < limit) return w % m;
    }
  }
  HFr field() {  // eight words as a little-endian 512-bit integer, reduced mod r
    uint64_t lo[4], hi[4];
    for (auto& w : lo) w = next();
    for (auto& w : hi) w = next();
    uint8_t b[32];
    memcpy(b, lo, 32);
    const HFr l = host::fr_mod_from_le_bytes(b);
    memcpy(b, hi, 32);
    const HFr hh = host::fr_mod_from_le_bytes(b);
    const HFr two256 = HFr::from_canonical(host::FrTag::R1);  // 2^256 mod r
    return l + hh * two256;
  }
};

void sample(WordStream& ws, BdMatrix& mat) {  // SparseMatrix::new (code/brakedown.rs:279-297)
  const BdDim& d = mat.dim;
  mat.cols.resize(d.n * d.d);
  mat.coeffs.resize(d.n * d.d);
  std::vector<uint32_t> cols;
  for (size_t i = 0; i < d.n; i++) {
    cols.clear();
    while (cols.size() < d.d) {
      const uint32_t c = (uint32_t)ws.uniform(d.m);
      if (std::find(cols.begin(), cols.end(), c) == cols.end()) cols.push_back(c);
    }
    std::sort(cols.begin(), cols.end());
    for (size_t k = 0; k < d.d; k++) {
      mat.cols[i * d.d + k] = cols[k];
      mat.coeffs[i * d.d + k] = ws.field();
    }
  }
}

void upload(Ctx& c, BdMatrix& mat) {  // transposed CSR, grouped by output index, inputs ascending
  const BdDim& d = mat.dim;
  std::vector<uint32_t> ptr(d.m + 1, 0), idx(d.n * d.d);
  std::vector<HFr> val(d.n * d.d);
  for (uint32_t col : mat.cols) ptr[col + 1]++;
  for (size_t j = 0; j < d.m; j++) ptr[j + 1] += ptr[j];
  std::vector<uint32_t> fill(ptr.begin(), ptr.end() - 1);
  for (size_t i = 0; i < d.n; i++)
    for (size_t k = 0; k < d.d; k++) {
      const uint32_t e = fill[mat.cols[i * d.d + k]]++;
      idx[e] = (uint32_t)i;
      val[e] = mat.coeffs[i * d.d + k];
    }
  mat.mem[0].alloc(ptr.size() * 4);
  mat.mem[1].alloc(std::max<size_t>(idx.size(), 1) * 4);
  mat.mem[2].alloc(std::max<size_t>(val.size(), 1) * 32);
  mat.d_ptr = mat.mem[0], mat.d_idx = mat.mem[1], mat.d_val = mat.mem[2];
  LH_HIP(hipMemcpyAsync(mat.d_ptr, ptr.data(), ptr.size() * 4, hipMemcpyHostToDevice, c.stream));
  if (!idx.empty()) {
    LH_HIP(hipMemcpyAsync(mat.d_idx, idx.data(), idx.size() * 4, hipMemcpyHostToDevice, c.stream));
    LH_HIP(hipMemcpyAsync(mat.d_val, val.data(), val.size() * 32, hipMemcpyHostToDevice, c.stream));
  }
  c.sync();
}
}  // namespace

void brakedown_derive(BdParam& p, size_t num_vars, int spec) {
  LH_REQUIRE(spec >= 1 && spec <= 6, LH_ERR_ARG, "brakedown: spec must be 1..6");
  LH_REQUIRE(num_vars >= 1 && num_vars <= 40, LH_ERR_ARG, "brakedown: num_vars must be 1..40");
  const Spec& s = SPECS[spec - 1];
  p.spec = spec, p.num_vars = num_vars;
  p.n_0 = std::min<size_t>(20, ((size_t)1 << num_vars) - 1);  // brakedown.rs:102
  size_t best = SIZE_MAX, row_len = 0;
  for (size_t log2_n = log2_ceil(p.n_0 + 1); log2_n <= num_vars; log2_n++) {  // Brakedown::new_multilinear
    const size_t ps = proof_size(s, p.n_0, (size_t)1 << log2_n, (size_t)1 << (num_vars - log2_n));
    if (ps < best) best = ps, row_len = (size_t)1 << log2_n;
  }
  p.row_len = row_len;
  p.num_rows = ((size_t)1 << num_vars) / row_len;
  std::vector<BdDim> a, b;
  dimensions(s, row_len, p.n_0, a, b);
  p.a = std::vector<BdMatrix>(a.size());
  p.b = std::vector<BdMatrix>(b.size());
  for (size_t k = 0; k < a.size(); k++) p.a[k].dim = a[k], p.b[k].dim = b[k];
  p.codeword_len = codeword_len(s, row_len, p.n_0);
  p.num_column_opening = num_column_opening(s);
  p.num_proximity_testing = num_proximity_testing(s, row_len, p.n_0);
  p.depth = log2_ceil(p.codeword_len);
  LH_REQUIRE(p.codeword_len < ((size_t)1 << 32), LH_ERR_ARG, "brakedown: codeword too long");
}

BdParam brakedown_setup(Ctx* c, size_t num_vars, int spec, const uint8_t seed[32]) {
  BdParam p;
  brakedown_derive(p, num_vars, spec);
  WordStream ws;
  memcpy(ws.seed, seed, 32);
  for (size_t k = 0; k < p.a.size(); k++) sample(ws, p.a[k]), sample(ws, p.b[k]);  // a[0], b[0], a[1], b[1], ..
  if (c) {
    p.device = c->device;
    for (size_t k = 0; k < p.a.size(); k++) upload(*c, p.a[k]), upload(*c, p.b[k]);
  }
  return p;
}

// ------------------------------------------------------------------ Ligero: the Reed-Solomon code (tests/ligero_ref.py)
namespace {
// num_column_opening of a code of relative distance 1 - 2^-b, the reference's formula in IEEE double
size_t rs_num_column_opening(int b) {
  const double delta = 1.0 - 1.0 / (double)((size_t)1 << b);
  return ceil_(-LAMBDA / log2(1.0 - delta / 3.0));
}
size_t rs_num_proximity_testing(size_t log2_n) { return ceil_(LAMBDA / ((double)LOG2_Q - (double)log2_n)); }

// w_(2^28) = 7^((r - 1) / 2^28), raised to 2^(28 - log2_m)
HFr root_of_unity(size_t log2_m) {
  uint64_t e[4];
  memcpy(e, host::FrTag::MOD, 32);
  e[0] -= 1;
  for (int i = 0; i < 4; i++) e[i] = (e[i] >> 28) | (i < 3 ? e[i + 1] << 36 : 0);
  HFr w = HFr::from_u64(7).pow(e);
  for (size_t k = log2_m; k < 28; k++) w = w.sqr();
  return w;
}

// in place, natural order in and out: x[s] <- sum_t x[t] w^(+-ts), w = tw[step]; tw has `m * step` entries of period m * step
void host_ntt(HFr* x, size_t log2_m, const HFr* tw, size_t step, bool inverse) {
  const size_t m = (size_t)1 << log2_m, period = m * step;
  for (size_t i = 0, j = 0; i < m; i++) {  // bit reversal
    if (i < j) std::swap(x[i], x[j]);
    size_t bit = m >> 1;
    for (; bit && (j & bit); bit >>= 1) j ^= bit;
    j |= bit;
  }
  for (size_t h = 1; h < m; h <<= 1) {
    const size_t ts = period / (2 * h);
    for (size_t g = 0; g < m; g += 2 * h)
      for (size_t k = 0; k < h; k++) {
        const HFr& w = tw[inverse ? (period - k * ts) & (period - 1) : k * ts];
        const HFr u = x[g + k], v = x[g + k + h] * w;
        x[g + k] = u + v, x[g + k + h] = u - v;
      }
  }
}

void rs_encode_host(const BdParam& p, HFr* t) {
  LH_REQUIRE(p.tw.size() == p.codeword_len, LH_ERR_ARG, "ligero: parameters without the table of roots");
  const size_t K = p.row_len, N = p.codeword_len, k = p.depth - (size_t)p.log_inv_rate, cosets = N / K;
  std::vector<HFr> f(t, t + K);
  host_ntt(f.data(), k, p.tw.data(), cosets, true);
  const HFr k_inv = HFr::from_u64(K).inv();
  for (HFr& v : f) v *= k_inv;
  for (size_t i = 1; i < cosets; i++) {  // f(w_N^i x) on the K-th roots: coefficient t scaled by w_N^(i t)
    HFr* out = t + i * K;
    for (size_t j = 0; j < K; j++) out[j] = f[j] * p.tw[(i * j) & (N - 1)];
    host_ntt(out, k, p.tw.data(), cosets, false);
  }
}
}  // namespace

void ligero_derive(BdParam& p, size_t num_vars, int b, size_t row_vars) {
  LH_REQUIRE(b >= 1 && b <= 3, LH_ERR_ARG, "ligero: log_inv_rate must be 1..3");
  LH_REQUIRE(num_vars >= 1 && num_vars <= 26, LH_ERR_ARG, "ligero: num_vars must be 1..26");
  LH_REQUIRE(row_vars == LIGERO_ROW_VARS_AUTO || row_vars <= num_vars, LH_ERR_ARG, "ligero: row_vars exceeds num_vars");
  const size_t t = rs_num_column_opening(b);
  if (row_vars == LIGERO_ROW_VARS_AUTO) {
    size_t best = SIZE_MAX;
    for (size_t rv = 0; rv <= num_vars; rv++) {  // the smallest proof; the smallest row on a tie
      const size_t ps = (1 + rs_num_proximity_testing(rv + b)) * ((size_t)1 << rv) + t * ((size_t)1 << (num_vars - rv));
      if (ps < best) best = ps, row_vars = rv;
    }
  }
  LH_REQUIRE(row_vars + (size_t)b <= 28, LH_ERR_ARG, "ligero: the codeword exceeds the field's 2^28 roots of unity");
  p.code = BD_CODE_RS, p.log_inv_rate = b, p.spec = 0, p.num_vars = num_vars, p.n_0 = 0;
  p.row_len = (size_t)1 << row_vars;
  p.num_rows = (size_t)1 << (num_vars - row_vars);
  p.depth = row_vars + (size_t)b;
  p.codeword_len = (size_t)1 << p.depth;
  p.num_column_opening = t;
  p.num_proximity_testing = rs_num_proximity_testing(p.depth);
}

BdParam ligero_setup(Ctx* c, size_t num_vars, int b, size_t row_vars) {
  BdParam p;
  ligero_derive(p, num_vars, b, row_vars);
  const HFr w = root_of_unity(p.depth);
  p.tw.resize(p.codeword_len);
  p.tw[0] = HFr::one();
  for (size_t i = 1; i < p.codeword_len; i++) p.tw[i] = p.tw[i - 1] * w;
  if (c) {
    p.device = c->device;
    p.tw_mem.alloc(p.tw.size() * sizeof(Fr));
    p.d_tw = p.tw_mem;
    LH_HIP(hipMemcpyAsync(p.d_tw, p.tw.data(), p.tw.size() * sizeof(Fr), hipMemcpyHostToDevice, c->stream));
    c->sync();
  }
  return p;
}

void brakedown_trim(const BdParam& p, size_t poly_size) {
  LH_REQUIRE(poly_size && !(poly_size & (poly_size - 1)), LH_ERR_ARG, "brakedown: poly_size must be a power of two");
  LH_REQUIRE(poly_size == ((size_t)1 << p.num_vars), LH_ERR_INVALID_PCS_PARAM,
             "Can't trim MultilinearBrakedownParams into different poly_size");
}

// ------------------------------------------------------------------ host encoder (code/brakedown.rs:88-125)
static void dot_into(const BdMatrix& mat, const HFr* in, HFr* out) {
  const size_t d = mat.dim.d;
  for (size_t i = 0; i < mat.dim.n; i++)
    for (size_t k = 0; k < d; k++) out[mat.cols[i * d + k]] += in[i] * mat.coeffs[i * d + k];
}

void brakedown_encode_host(const BdParam& p, HFr* t) {
  if (p.code == BD_CODE_RS) return rs_encode_host(p, t);
  LH_REQUIRE(!p.a.empty() && p.a[0].cols.size() == p.a[0].dim.n * p.a[0].dim.d, LH_ERR_ARG,
             "brakedown: parameters without matrices");
  for (size_t i = p.row_len; i < p.codeword_len; i++) t[i] = HFr::zero();
  size_t in_off = 0;
  for (size_t k = 0; k + 1 < p.a.size(); k++) {
    dot_into(p.a[k], t + in_off, t + in_off + p.a[k].dim.n);
    in_off += p.a[k].dim.n;
  }
  const BdMatrix &al = p.a.back(), &bl = p.b.back();
  std::vector<HFr> tmp(al.dim.m, HFr::zero());
  dot_into(al, t + in_off, tmp.data());
  for (size_t x = 0; x < bl.dim.n; x++) {  // reed_solomon_into: horner(tmp, x) at x = 1, 2, ..
    const HFr xv = HFr::from_u64(x + 1);
    HFr acc = HFr::zero();
    for (size_t k = tmp.size(); k-- > 0;) acc = acc * xv + tmp[k];
    t[in_off + al.dim.n + x] = acc;
  }
  size_t out_off = in_off + al.dim.n + bl.dim.n;
  in_off += al.dim.n + al.dim.m;
  for (size_t k = p.a.size(); k-- > 0;) {
    in_off -= p.a[k].dim.m;
    dot_into(p.b[k], t + in_off, t + out_off);
    out_off += p.b[k].dim.m;
  }
}

// ------------------------------------------------------------------ commit (brakedown.rs:130-206)
static void check_vars(const BdParam& p, size_t num_vars, const char* what) {
  if (num_vars != p.num_vars)  // validate_input (pcs/multilinear.rs:27-70) at the only size a Brakedown param takes
    throw Error(LH_ERR_INVALID_PCS_PARAM, std::string("Invalid poly or point to ") + what + " (param supports " +
                                              std::to_string(p.num_vars) + " variates but got " +
                                              std::to_string(num_vars) + ")");
}

// the cascade over `R` rows that hold their messages: a[k] forward, the Reed-Solomon tail, b[k] in reverse
// (`first_done`: a[0]'s outputs are already there - the column commit's u32 gather)
static void encode_rows(Ctx& c, const BdParam& p, Fr* rows, size_t R, bool first_done = false) {
  const size_t cw = p.codeword_len;
  if (p.code == BD_CODE_RS) {  // one code, no cascade: kernels_ntt.hip
    LH_REQUIRE(p.d_tw && !first_done, LH_ERR_ARG, "ligero: parameters were set up without a device");
    return k_bd_rs_encode(c, rows, R, cw, p.depth - (size_t)p.log_inv_rate, p.log_inv_rate, p.d_tw);
  }
  size_t in_off = 0;
  for (size_t k = 0; k + 1 < p.a.size(); k++) {
    if (k || !first_done) k_bd_gather(c, rows, R, cw, in_off, in_off + p.a[k].dim.n, p.a[k]);
    in_off += p.a[k].dim.n;
  }
  const BdMatrix &al = p.a.back(), &bl = p.b.back();
  k_bd_reed_solomon(c, rows, R, cw, in_off, al, bl.dim.n);
  size_t out_off = in_off + al.dim.n + bl.dim.n;
  in_off += al.dim.n + al.dim.m;
  for (size_t k = p.a.size(); k-- > 0;) {
    in_off -= p.a[k].dim.m;
    k_bd_gather(c, rows, R, cw, in_off, out_off, p.b[k]);
    out_off += p.b[k].dim.m;
  }
  LH_REQUIRE(in_off == p.row_len && out_off == cw, LH_ERR_ARG, "brakedown: cascade does not tile the codeword");
}

std::unique_ptr<BdComm> brakedown_commit(Ctx& c, const BdParam& p, const Fr* d_poly, size_t num_vars) {
  check_vars(p, num_vars, "commit");
  LH_REQUIRE(p.device == c.device, LH_ERR_ARG, "brakedown: parameters were not set up on this ctx's device");
  const size_t R = p.num_rows, cw = p.codeword_len, width = (size_t)1 << p.depth;
  std::unique_ptr<BdComm> comm(new BdComm());
  comm->num_rows = R, comm->codeword_len = cw, comm->depth = p.depth, comm->device = c.device;
  comm->rows_mem.alloc(R * cw * sizeof(Fr));
  comm->hashes_mem.alloc(((2 * width) - 1) * 32);
  Fr* rows = comm->d_rows = comm->rows_mem;
  comm->d_hashes = comm->hashes_mem;
  // row r's message is poly[r * row_len ..]
  LH_HIP(hipMemcpy2DAsync(rows, cw * sizeof(Fr), d_poly, p.row_len * sizeof(Fr), p.row_len * sizeof(Fr), R,
                          hipMemcpyDeviceToDevice, c.stream));
  encode_rows(c, p, rows, R);
  // column leaves, then one launch per tree level
  k_bd_hash_columns(c, rows, R, cw, width, comm->d_hashes);
  size_t off = 0;
  for (size_t w = width; w > 1; w >>= 1) {
    k_bd_merkle_level(c, comm->d_hashes + 4 * off, w / 2, comm->d_hashes + 4 * (off + w));
    off += w;
  }
  c.d2h(comm->root, comm->d_hashes + 4 * off, 32);
  return comm;
}

// ------------------------------------------------------------------ batch commit: P polys, the launches of one
// The slab: P * num_rows rows of codeword_len, then P trees of (2 << depth) - 1 digests, then P roots gathered for the copy.
static size_t batch_rows_bytes(const BdParam& p, size_t P) {
  return (P * p.num_rows * p.codeword_len * sizeof(Fr) + 255) & ~(size_t)255;
}
static size_t batch_tree_words(const BdParam& p) { return 4 * (((size_t)2 << p.depth) - 1); }
static std::vector<std::unique_ptr<BdComm>> batch_trees(Ctx& c, const BdParam& p, size_t P, Fr* rows, uint64_t* trees,
                                                        uint64_t* d_roots, const std::shared_ptr<DevMem>& owner);
// the slab of a batch: the caller's memory, or (null) one allocation that the batch's commitments share
struct BatchSlab {
  std::shared_ptr<DevMem> owner;
  char* mem;
  BatchSlab(void* given, size_t bytes) : mem((char*)given) {
    if (!given) owner = std::make_shared<DevMem>(bytes), mem = owner->as<char>();
  }
};
size_t brakedown_batch_bytes(const BdParam& p, size_t P) {
  return batch_rows_bytes(p, P) + ((P * batch_tree_words(p) * 8 + 255) & ~(size_t)255) + ((P * 32 + 255) & ~(size_t)255) +
         ((P * sizeof(Fr*) + 255) & ~(size_t)255);
}

std::vector<std::unique_ptr<BdComm>> brakedown_batch_commit(Ctx& c, const BdParam& p, const Fr* const* d_polys, size_t P,
                                                            size_t num_vars, void* slab_mem) {
  if (!P) return {};
  check_vars(p, num_vars, "commit");
  LH_REQUIRE(p.device == c.device, LH_ERR_ARG, "brakedown: parameters were not set up on this ctx's device");
  const size_t R = p.num_rows, cw = p.codeword_len, tree_words = batch_tree_words(p);
  const BatchSlab slab(slab_mem, brakedown_batch_bytes(p, P));
  Fr* rows = (Fr*)slab.mem;
  uint64_t* trees = (uint64_t*)(slab.mem + batch_rows_bytes(p, P));
  uint64_t* d_roots = (uint64_t*)((char*)trees + ((P * tree_words * 8 + 255) & ~(size_t)255));
  const Fr** d_ptrs = (const Fr**)((char*)d_roots + ((P * 32 + 255) & ~(size_t)255));
  LH_HIP(hipMemcpyAsync(d_ptrs, d_polys, P * sizeof(Fr*), hipMemcpyHostToDevice, c.stream));
  k_bd_load_rows(c, d_ptrs, P, R, p.row_len, cw, rows);
  encode_rows(c, p, rows, P * R);  // (rows are independent: the slab is P * R of them)
  return batch_trees(c, p, P, rows, trees, d_roots, slab.owner);
}

// the column leaves, the trees and the roots of a slab whose P * num_rows rows are encoded -> the P commitments
static std::vector<std::unique_ptr<BdComm>> batch_trees(Ctx& c, const BdParam& p, size_t P, Fr* rows, uint64_t* trees,
                                                        uint64_t* d_roots, const std::shared_ptr<DevMem>& owner) {
  const size_t R = p.num_rows, cw = p.codeword_len, width = (size_t)1 << p.depth, tree_words = batch_tree_words(p);
  std::vector<std::unique_ptr<BdComm>> comms;
  k_bd_hash_columns_batch(c, rows, P, R, cw, width, trees, tree_words);
  size_t off = 0;
  for (size_t w = width; w > 1; w >>= 1) {
    k_bd_merkle_level_batch(c, trees, P, tree_words, 4 * off, w / 2, 4 * (off + w));
    off += w;
  }
  k_bd_gather_roots(c, trees, P, tree_words, 4 * off, d_roots);
  std::vector<uint8_t> roots(32 * P);
  c.d2h(roots.data(), d_roots, 32 * P);  // (synchronises: the caller's pointer table has been read by then)
  for (size_t i = 0; i < P; i++) {
    std::unique_ptr<BdComm> comm(new BdComm());
    comm->num_rows = R, comm->codeword_len = cw, comm->depth = p.depth, comm->device = c.device;
    comm->d_rows = rows + i * R * cw, comm->d_hashes = trees + i * tree_words;
    comm->slab = owner, comm->borrowed = !owner;
    memcpy(comm->root, roots.data() + 32 * i, 32);
    comms.push_back(std::move(comm));
  }
  return comms;
}

// ------------------------------------------------------------------ column commit: the batch without a table per column
// The slab of a batch, its pointer table replaced by the column table.
size_t brakedown_columns_bytes(const BdParam& p, size_t P) {
  return batch_rows_bytes(p, P) + ((P * batch_tree_words(p) * 8 + 255) & ~(size_t)255) + ((P * 32 + 255) & ~(size_t)255) +
         ((P * sizeof(BdColumn) + 255) & ~(size_t)255);
}

std::vector<std::unique_ptr<BdComm>> brakedown_commit_columns(Ctx& c, const BdParam& p, const BdColumn* cols, size_t P,
                                                              void* slab_mem) {
  if (!P) return {};
  LH_REQUIRE(p.device == c.device, LH_ERR_ARG, "brakedown: parameters were not set up on this ctx's device");
  bool any_u32 = false, any_fr = false;
  for (size_t i = 0; i < P; i++) {
    LH_REQUIRE(cols[i].len <= ((uint64_t)1 << p.num_vars), LH_ERR_ARG, "brakedown: a column is longer than 2^num_vars");
    LH_REQUIRE(cols[i].data || !cols[i].len, LH_ERR_ARG, "brakedown: null column");
    (cols[i].u32 ? any_u32 : any_fr) = true;
  }
  const size_t R = p.num_rows, cw = p.codeword_len, tree_words = batch_tree_words(p);
  const BatchSlab slab(slab_mem, brakedown_columns_bytes(p, P));
  Fr* rows = (Fr*)slab.mem;
  uint64_t* trees = (uint64_t*)(slab.mem + batch_rows_bytes(p, P));
  uint64_t* d_roots = (uint64_t*)((char*)trees + ((P * tree_words * 8 + 255) & ~(size_t)255));
  BdColumn* d_cols = (BdColumn*)((char*)d_roots + ((P * 32 + 255) & ~(size_t)255));
  LH_HIP(hipMemcpyAsync(d_cols, cols, P * sizeof(BdColumn), hipMemcpyHostToDevice, c.stream));
  k_bd_load_columns(c, d_cols, P, R, p.row_len, cw, rows);
  // a[0] of the u32 columns from their 4-byte entries (there is an a[0] outside the Reed-Solomon tail when the cascade has
  // more than one level); the field-element columns among them keep bd_gather, a column at a time
  // (a Reed-Solomon param has no a[0]: load, then encode, whatever the option says)
  const bool u32_first = p.code == BD_CODE_EXPANDER && c.opt.brakedown_u32_gather != 0 && any_u32 && p.a.size() > 1;
  if (u32_first) {
    k_bd_gather_u32(c, d_cols, P, rows, R, p.row_len, cw, p.a[0]);
    if (any_fr)
      for (size_t i = 0; i < P; i++)
        if (!cols[i].u32) k_bd_gather(c, rows + i * R * cw, R, cw, 0, p.row_len, p.a[0]);
  }
  encode_rows(c, p, rows, P * R, u32_first);
  return batch_trees(c, p, P, rows, trees, d_roots, slab.owner);  // (synchronises: the caller's table has been read by then)
}

// ------------------------------------------------------------------ open (brakedown.rs:212-276)
void brakedown_stage(Ctx& c, const BdParam& p, const BdComm& comm, BdStage& st) {
  LH_REQUIRE(comm.num_rows == p.num_rows && comm.codeword_len == p.codeword_len && comm.device == c.device, LH_ERR_ARG,
             "brakedown: commitment does not belong to these parameters");
  if (st.of == &comm) return;
  const size_t R = p.num_rows, cw = p.codeword_len, bytes = R * cw * sizeof(Fr);
  st.of = nullptr;
  st.cols.reserve(bytes);
  if (R == 1) {  // the row is its own transpose
    LH_HIP(hipMemcpyAsync(st.cols, comm.d_rows, bytes, hipMemcpyDeviceToHost, c.stream));
    c.sync();
  } else {
    ArenaScope scope(c.arena);
    Fr* t = c.arena.alloc_n<Fr>(R * cw);
    k_bd_stage_columns(c, comm.d_rows, R, cw, t);
    LH_HIP(hipMemcpyAsync(st.cols, t, bytes, hipMemcpyDeviceToHost, c.stream));
    c.sync();
  }
  st.of = &comm;
}

void brakedown_open(Ctx& c, const BdParam& p, const Fr* d_poly, size_t num_vars, BdComm& comm, const HFr* point,
                    Transcript& tr, HashTranscript& ht, const BdStage* staged) {
  check_vars(p, num_vars, "open");
  LH_REQUIRE(!staged || staged->of == &comm, LH_ERR_ARG, "brakedown: the staged matrix is another commitment's");
  LH_REQUIRE(comm.num_rows == p.num_rows && comm.codeword_len == p.codeword_len && comm.device == c.device, LH_ERR_ARG,
             "brakedown: commitment does not belong to these parameters");
  const size_t R = p.num_rows, row_len = p.row_len, cw = p.codeword_len, k_rows = log2_ceil(R);
  // without a table the polynomial is the message part of the commitment's rows: the same values, row stride codeword_len
  const size_t stride = d_poly ? row_len : cw;
  if (!d_poly) d_poly = comm.d_rows;
  ArenaScope scope(c.arena);
  std::vector<HFr> row(row_len);
  if (R > 1) {
    // point_to_tensor: (hi, lo) split at len - log2(num_rows); t_0 = eq(lo) weighs the rows
    const std::vector<HFr> t_0 = host_eq_xy(std::vector<HFr>(point + num_vars - k_rows, point + num_vars));
    Fr* coeffs = c.arena.alloc_n<Fr>(2 * R);
    Fr* out = c.arena.alloc_n<Fr>(2 * row_len);
    std::vector<HFr> both(2 * row_len);
    for (size_t k = 0; k < p.num_proximity_testing; k++) {
      const std::vector<HFr> cs = tr.squeeze_challenges(R);
      const bool last = k + 1 == p.num_proximity_testing;  // the last proximity row and the t_0 row share one pass
      LH_HIP(hipMemcpyAsync(coeffs, cs.data(), R * 32, hipMemcpyHostToDevice, c.stream));
      if (last) LH_HIP(hipMemcpyAsync(coeffs + R, t_0.data(), R * 32, hipMemcpyHostToDevice, c.stream));
      k_bd_combine(c, d_poly, R, row_len, stride, coeffs, last ? 2 : 1, out);
      c.d2h(both.data(), out, (last ? 2 : 1) * row_len * 32);
      tr.write_field_elements(std::vector<HFr>(both.begin(), both.begin() + row_len));
    }
    std::copy(both.begin() + row_len, both.end(), row.begin());
  } else {
    c.d2h(row.data(), d_poly, row_len * 32);  // num_rows == 1: the t_0 row is the polynomial itself
  }
  tr.write_field_elements(row);

  // the paths are read from a host copy of the tree; each column is fetched as it is squeezed (the next index depends on
  // the entries this one absorbs)
  if (comm.host_tree.empty()) {
    comm.host_tree.resize(4 * ((2 << p.depth) - 1));
    c.d2h(comm.host_tree.data(), comm.d_hashes, comm.host_tree.size() * 8);
  }
  HFr* col = staged ? nullptr : (HFr*)c.pin(R * 32);
  std::vector<HFr> items(R);
  for (size_t i = 0; i < p.num_column_opening; i++) {
    uint8_t repr[32];
    tr.squeeze_challenge().to_repr(repr);  // squeeze_challenge_idx (brakedown.rs:427-435)
    const size_t column = (size_t)(((uint32_t)repr[0] | (uint32_t)repr[1] << 8 | (uint32_t)repr[2] << 16 |
                                    (uint32_t)repr[3] << 24) % cw);
    if (staged) {
      col = staged->cols.as<HFr>() + column * R;
    } else {
      LH_HIP(hipMemcpy2DAsync(col, 32, comm.d_rows + column, cw * sizeof(Fr), 32, R, hipMemcpyDeviceToHost, c.stream));
      c.sync();
    }
    items.assign(col, col + R);
    tr.write_field_elements(items);
    size_t offset = 0;
    for (size_t idx = 0; idx < p.depth; idx++) {
      ht.write_hash((const uint8_t*)(comm.host_tree.data() + 4 * (offset + ((column >> idx) ^ 1))));
      offset += (size_t)1 << (p.depth - idx);
    }
  }
}

// ------------------------------------------------------------------ the provers' PCS (backend/hyperplonk.rs:76-95)
namespace {
struct BdStore {
  std::map<const void*, BdComm*> by_poly;  // (a table's pointer, or a u32 column's)
  std::vector<std::unique_ptr<BdComm>> own;  // (views into arena slabs of the proof's scope: nothing to free on the device)
  BdStage stage;
};
}  // namespace

Pcs brakedown_pcs(Ctx& c, const BdParam& p, HashTranscript& ht, const std::vector<BdGiven>& given) {
  std::shared_ptr<BdStore> store(new BdStore());
  for (const BdGiven& g : given) {
    LH_REQUIRE(g.d_poly && g.comm, LH_ERR_ARG, "brakedown: null poly or commitment");
    store->by_poly[g.d_poly] = g.comm;
  }
  Pcs pcs;
  pcs.max_vars = p.num_vars;
  pcs.commit_and_write = [&c, &p, &ht, store](const Fr* const* polys, size_t np, size_t nv, Transcript&) {
    if (!np) return;
    void* slab = c.arena.alloc(brakedown_batch_bytes(p, np));  // released with the prove's ArenaScope
    std::vector<std::unique_ptr<BdComm>> comms = brakedown_batch_commit(c, p, polys, np, nv, slab);
    for (size_t i = 0; i < np; i++) {
      ht.write_hash(comms[i]->root);
      store->by_poly[polys[i]] = comms[i].get();
      store->own.push_back(std::move(comms[i]));
    }
  };
  pcs.commit_columns_and_write = [&c, &p, &ht, store](const PcsColumn* cols, size_t nc, size_t nv, Transcript&) {
    check_vars(p, nv, "commit");
    std::vector<BdColumn> uniq;  // (a column handed over twice - E of an identity subtable is dim - is committed once)
    std::vector<size_t> slot(nc);
    for (size_t i = 0; i < nc; i++) {
      LH_REQUIRE(cols[i].data, LH_ERR_ARG, "brakedown commit_columns: null column");
      size_t k = 0;
      while (k < uniq.size() && uniq[k].data != cols[i].data) k++;
      if (k == uniq.size()) uniq.push_back(BdColumn{cols[i].data, cols[i].len, cols[i].u32 ? 1u : 0u, 0});
      LH_REQUIRE(uniq[k].len == cols[i].len, LH_ERR_ARG, "brakedown commit_columns: one column under two lengths");
      slot[i] = k;
    }
    if (uniq.empty()) return;
    void* slab = c.arena.alloc(brakedown_columns_bytes(p, uniq.size()));  // released with the prove's ArenaScope
    std::vector<std::unique_ptr<BdComm>> comms = brakedown_commit_columns(c, p, uniq.data(), uniq.size(), slab);
    for (size_t i = 0; i < nc; i++) ht.write_hash(comms[slot[i]]->root);
    for (size_t k = 0; k < uniq.size(); k++) {
      store->by_poly[uniq[k].data] = comms[k].get();
      store->own.push_back(std::move(comms[k]));
    }
  };
  pcs.batch_open = [&c, &p, &ht, store](size_t nv, const Fr* const* polys, size_t np, const HFr* points, size_t npts,
                                        const lh_evaluation* evals, size_t ne, Transcript& tr, const SmallPoly* small) {
    // (the stage holds ONE matrix, the last commitment's: HyperPlonk's evaluations come poly-major, so a poly queried at
    // several points is staged once; Lasso's _evals order - a, E at r_z, dim, read_ts, E at r_N, final_cts - comes back to
    // every E, and under an identity subtable to every dim, so those matrices are staged again: 1 + 3 c + 2 alpha stagings
    // for 1 + 3 c + alpha commitments or fewer.  A stage per commitment would pin all of a proof's matrices at once.)
    for (size_t i = 0; i < ne; i++) {
      const lh_evaluation& e = evals[i];
      LH_REQUIRE(e.poly < np && e.point < npts, LH_ERR_ARG, "brakedown batch_open: evaluation out of range");
      // a poly that came as a u32 column was committed under the column's pointer and has no table to combine from
      const bool by_column = small && small[e.poly].ptr && store->by_poly.count(small[e.poly].ptr);
      LH_REQUIRE(by_column || polys[e.poly], LH_ERR_ARG, "brakedown batch_open: evaluation out of range");
      auto it = store->by_poly.find(by_column ? (const void*)small[e.poly].ptr : (const void*)polys[e.poly]);
      LH_REQUIRE(it != store->by_poly.end(), LH_ERR_ARG, "brakedown batch_open: no commitment for an opened poly");
      brakedown_stage(c, p, *it->second, store->stage);
      brakedown_open(c, p, by_column ? nullptr : polys[e.poly], nv, *it->second, points + (size_t)e.point * nv, tr, ht,
                     &store->stage);
    }
  };
  return pcs;
}

void brakedown_hyperplonk_prove_phases(Ctx& c, const BdParam& p, const lh_hp_param& pp, BdComm* const* preprocess_comms,
                                       BdComm* const* permutation_comms, const HpPhases& ph, const HFr* const* instances,
                                       Transcript& tr, HashTranscript& ht) {
  LH_REQUIRE(pp.num_lasso_lookups == 0, LH_ERR_ARG,
             "hyperplonk over brakedown: Lasso lookups are not supported (their column commitments are points)");
  LH_REQUIRE(!Shard(c).on, LH_ERR_ARG, "hyperplonk over brakedown: sharded proves are not supported");
  LH_REQUIRE(pp.num_vars == p.num_vars, LH_ERR_ARG,
             "hyperplonk over brakedown: the circuit has " + std::to_string(pp.num_vars) + " variables, the param " +
                 std::to_string(p.num_vars));
  LH_REQUIRE(p.device == c.device, LH_ERR_ARG, "brakedown: parameters were not set up on this ctx's device");
  std::vector<BdGiven> given;
  for (size_t i = 0; i < pp.num_preprocess_polys; i++) {
    LH_REQUIRE(pp.d_preprocess_polys && pp.d_preprocess_polys[i] && preprocess_comms[i], LH_ERR_ARG,
               "null argument: preprocess poly or commitment");
    given.push_back(BdGiven{(const Fr*)pp.d_preprocess_polys[i], preprocess_comms[i]});
  }
  for (size_t i = 0; i < pp.num_permutation_polys; i++) {
    LH_REQUIRE(pp.d_permutation_polys && pp.d_permutation_polys[i] && permutation_comms[i], LH_ERR_ARG,
               "null argument: permutation poly or commitment");
    given.push_back(BdGiven{(const Fr*)pp.d_permutation_polys[i], permutation_comms[i]});
  }
  const Pcs pcs = brakedown_pcs(c, p, ht, given);  // (dies with this frame, also when the prove throws)
  hyperplonk_prove_phases(c, pcs, pp, ph, instances, tr);
}

void brakedown_lasso_prove(Ctx& c, const BdParam& p, const lh_lasso_table& tb, size_t num_vars, const uint32_t* const* d_dims,
                           Transcript& tr, HashTranscript& ht) {
  lasso_check_table(tb);
  LH_REQUIRE(!Shard(c).on, LH_ERR_ARG, "lasso over brakedown: sharded proves are not supported");
  LH_REQUIRE(p.num_vars == std::max<size_t>(num_vars, tb.chunk_bits), LH_ERR_ARG,
             "lasso over brakedown: the columns have max(num_vars, chunk_bits) = " +
                 std::to_string(std::max<size_t>(num_vars, tb.chunk_bits)) + " variables, the param " +
                 std::to_string(p.num_vars));
  LH_REQUIRE(p.device == c.device, LH_ERR_ARG, "brakedown: parameters were not set up on this ctx's device");
  const Pcs pcs = brakedown_pcs(c, p, ht, {});  // (dies with this frame, also when the prove throws)
  lasso_prove(c, pcs, tb, num_vars, d_dims, tr);
}

}  // namespace lh
