// The multilinear IPA over BN254 G1: parameters and prover half (reference pcs/multilinear/ipa.rs:98-254 with
// C = bn256::G1Affine).  An opening of an n-variable table is n rounds of
//   two inner products            one launch (k_ipa_cross)
//   L and R                       ONE msm_batch of two jobs over the round's bases; the h' terms are added on the host
//   the base fold                 bases_l += xi bases_r, affine again (k_g1_axpy)
//   two axpys                     coeffs_l += xi^-1 coeffs_r, zs_l += xi zs_r, one launch (k_ipa_fold_fr)
// and the last coefficient: 128 n + 32 bytes.  Everything lives in the arena; nothing is allocated inside an opening.
// The generators are the library's own hash-to-point under the reference's domain and messages (the reference's
// hash_to_curve comes from a curve-library branch whose bytes cannot be pinned): specified in DESIGN.md §14, restated in
// tests/ipa_ref.py, computed here on the host (verifier param, setup without a ctx) and in kernels_ipa.hip (prover bases).
#include <algorithm>
#include <memory>
#include "host.hpp"

namespace lh {

static const char IPA_DOMAIN[] = "MultilinearIpa::setup";  // ipa.rs:105,123

static host::Fq fq_from_u256(const uint8_t* le) {
  uint64_t c[4];
  memcpy(c, le, 32);
  while (host::Fq::geq_mod(c)) host::Fq::sub_mod(c);  // < 2^256 < 6 q
  return host::Fq::from_canonical(c);
}

HG1 ipa_hash_to_point(const uint8_t* message, size_t len) {
  static const host::Fq two256 = host::Fq{{host::FqTag::R2[0], host::FqTag::R2[1], host::FqTag::R2[2], host::FqTag::R2[3]}};
  static const host::Fq three = host::Fq::from_u64(3);
  uint64_t e[4];  // (q + 1) / 4
  for (int i = 0; i < 4; i++) {
    const uint64_t lo = host::FqTag::MOD[i] + (i == 0 ? 1 : 0), hi = i < 3 ? host::FqTag::MOD[i + 1] : 0;
    e[i] = (lo >> 2) | (hi << 62);
  }
  for (uint32_t ctr = 0;; ctr++) {
    uint8_t d[64];
    for (uint8_t tag = 0; tag < 2; tag++) {
      Keccak256 k;
      k.update((const uint8_t*)IPA_DOMAIN, sizeof(IPA_DOMAIN) - 1);
      k.update(message, len);
      const uint8_t tail[5] = {(uint8_t)ctr, (uint8_t)(ctr >> 8), (uint8_t)(ctr >> 16), (uint8_t)(ctr >> 24), tag};
      k.update(tail, 5);
      k.finalize_reset(d + 32 * tag);
    }
    const host::Fq x = fq_from_u256(d) + fq_from_u256(d + 32) * two256;
    const host::Fq rhs = x.sqr() * x + three;
    host::Fq y = rhs.pow(e);
    if (y.is_zero() || y.sqr() != rhs) continue;
    uint64_t canon[4];
    y.to_canonical(canon);
    if (canon[0] & 1) y = -y;
    return HG1{x, y};
  }
}

static HG1 ipa_generator_g(uint32_t idx) {  // ipa.rs:107-109
  const uint8_t m[5] = {0, (uint8_t)idx, (uint8_t)(idx >> 8), (uint8_t)(idx >> 16), (uint8_t)(idx >> 24)};
  return ipa_hash_to_point(m, 5);
}

static size_t log2_exact(size_t v, const char* what) {
  LH_REQUIRE(v >= 1 && (v & (v - 1)) == 0, LH_ERR_ARG, std::string(what) + ": poly_size is not a power of two");
  size_t k = 0;
  while (((size_t)1 << k) < v) k++;
  return k;
}

std::unique_ptr<IpaParams> ipa_setup(Ctx* c, size_t poly_size) {
  const size_t nv = log2_exact(poly_size, "ipa setup");
  LH_REQUIRE(nv >= 1 && nv <= 32, LH_ERR_ARG, "ipa setup: num_vars must be in 1..32");  // (h_coeffs asserts on 0, ipa.rs:320)
  std::unique_ptr<IpaParams> p(new IpaParams());
  p->num_vars = nv;
  const uint8_t one = 1;
  p->h = ipa_hash_to_point(&one, 1);  // ipa.rs:124
  if (c) {
    p->d_g.alloc(poly_size * sizeof(G1Affine));
    k_ipa_generators(*c, 0, poly_size, p->d_g);
    c->sync();
  } else {
    ipa_host_g(*p);
  }
  return p;
}

// the verifier's copy of g: a download when the bases are on a device (they were final when setup returned), derived on
// the host pool when not
const std::vector<HG1>& ipa_host_g(const IpaParams& p) {
  std::lock_guard<std::mutex> lk(p.mu);
  if (p.host_g.empty()) {
    std::vector<HG1> g((size_t)1 << p.num_vars);
    if (p.d_g) {
      OnDevice on(p.d_g.device());  // (the verifier entries take no ctx)
      LH_HIP(hipMemcpy(g.data(), p.d_g, g.size() * sizeof(HG1), hipMemcpyDeviceToHost));
      p.host_g.swap(g);
      return p.host_g;
    }
    // (chunks of 64: an item is ~4 Keccak permutations and ~1.5 exponentiations, about 100 us)
    const size_t chunk = 64, chunks = (g.size() + chunk - 1) / chunk;
    host_parallel_for(chunks, [&](size_t k) {
      for (size_t i = k * chunk; i < std::min(g.size(), (k + 1) * chunk); i++) g[i] = ipa_generator_g((uint32_t)i);
    });
    p.host_g.swap(g);
  }
  return p.host_g;
}

// ipa.rs:129-145 -> the trimmed param's num_vars
size_t ipa_trim_vars(const IpaParams& p, size_t poly_size) {
  const size_t nv = log2_exact(poly_size, "ipa trim");
  if (p.num_vars < nv)
    throw Error(LH_ERR_INVALID_PCS_PARAM, "Too many variates to trim (param supports variates up to " +
                                              std::to_string(p.num_vars) + " but got " + std::to_string(nv) + ")");
  LH_REQUIRE(nv >= 1, LH_ERR_ARG, "ipa trim: num_vars must be at least 1");
  return nv;
}
static void check_vars(size_t pp_vars, size_t num_vars, const char* what) {  // validate_input (pcs/multilinear.rs:26-70)
  if (pp_vars < num_vars)
    throw Error(LH_ERR_INVALID_PCS_PARAM, std::string("Too many variates of poly to ") + what + " (param supports variates up to " +
                                              std::to_string(pp_vars) + " but got " + std::to_string(num_vars) + ")");
}
static const G1Affine* device_g(const IpaParams& p) {
  LH_REQUIRE(p.d_g, LH_ERR_ARG, "ipa: the param was set up without a ctx (verifier param): it has no device bases");
  return p.d_g;
}

// ipa.rs:147-168; a poly of fewer variables is committed against a prefix of g (= its zero-padded table)
std::vector<HG1> ipa_batch_commit(Ctx& c, const IpaParams& p, size_t poly_size, const Fr* const* d_polys, size_t num_polys,
                                  size_t num_vars) {
  check_vars(ipa_trim_vars(p, poly_size), num_vars, num_polys == 1 ? "commit" : "batch commit");
  std::vector<HG1> out(num_polys);
  if (!num_polys) return out;
  const G1Affine* g = device_g(p);
  std::vector<MsmJob> jobs(num_polys);
  for (size_t i = 0; i < num_polys; i++) jobs[i] = MsmJob{d_polys[i], false, g, (size_t)1 << num_vars};
  msm_batch(c, jobs.data(), num_polys, (G1Affine*)out.data());
  return out;
}

static HG1 add_scaled(const HG1& p, const HG1& q, const HFr& s) {  // p + s q
  return host::g1_to_affine(host::g1_add(host::g1_from_affine(p), host::g1_mul(host::g1_from_affine(q), s)));
}

// ipa.rs:170-241
void ipa_open(Ctx& c, const IpaParams& p, size_t poly_size, const Fr* d_poly, size_t num_vars, const HFr* point, Transcript& tr) {
  const size_t pp_vars = ipa_trim_vars(p, poly_size);
  check_vars(pp_vars, num_vars, "open");
  // (the reference's round loop runs over the PARAM's variables and splits the poly's evaluations there: it panics otherwise)
  LH_REQUIRE(num_vars == pp_vars, LH_ERR_ARG, "ipa open: the poly must have as many variables as the (trimmed) param");
  const G1Affine* g = device_g(p);
  const size_t n = (size_t)1 << num_vars;
  const HFr xi_0 = tr.squeeze_challenge();
  const HG1 h_prime = host::g1_to_affine(host::g1_mul(host::g1_from_affine(p.h), xi_0));

  ArenaScope scope(c.arena);
  G1Affine* bases = c.arena.alloc_n<G1Affine>(n / 2);
  Fr* coeffs = c.arena.alloc_n<Fr>(n / 2);
  Fr* zs = c.arena.alloc_n<Fr>(n);
  Fr* cross = c.arena.alloc_n<Fr>(2 * IPA_CROSS_BLOCKS + 2);
  {
    std::vector<Fr> y(num_vars);
    for (size_t i = 0; i < num_vars; i++) y[i] = dev(point[i]);
    k_eq_xy(c, y.data(), num_vars, zs);
  }
  const G1Affine* cur_b = g;
  const Fr* cur_c = d_poly;
  for (size_t i = 0; i < num_vars; i++) {
    const size_t mid = (size_t)1 << (num_vars - i - 1);
    k_ipa_cross(c, cur_c, zs, mid, cross + 2, cross);
    const MsmJob jobs[2] = {MsmJob{cur_c + mid, false, cur_b, mid}, MsmJob{cur_c, false, cur_b + mid, mid}};
    HG1 lr[2];
    msm_batch(c, jobs, 2, (G1Affine*)lr);
    Fr cs[2];
    c.d2h(cs, cross, sizeof cs);
    tr.write_commitment(add_scaled(lr[0], h_prime, hst(cs[0])));  // the identity ends the opening here, as in the reference
    tr.write_commitment(add_scaled(lr[1], h_prime, hst(cs[1])));
    const HFr xi = tr.squeeze_challenge();
    LH_REQUIRE(!xi.is_zero(), LH_ERR_ARG, "ipa open: zero challenge (the reference unwraps its inverse)");
    k_g1_axpy(c, cur_b, cur_b + mid, mid, dev(xi), bases);
    k_ipa_fold_fr(c, cur_c, zs, mid, dev(xi.inv()), dev(xi), coeffs, zs);
    cur_b = bases, cur_c = coeffs;
  }
  Fr last;
  c.d2h(&last, cur_c, sizeof last);
  tr.write_field_element(hst(last));
}

void ipa_batch_open(Ctx& c, const IpaParams& p, size_t poly_size, size_t num_vars, const Fr* const* d_polys, size_t num_polys,
                    const HFr* points, size_t num_points, const lh_evaluation* evals, size_t num_evals, Transcript& tr,
                    const SmallPoly* small) {
  check_vars(ipa_trim_vars(p, poly_size), num_vars, "open");
  additive_batch_open(
      c, num_vars, d_polys, num_polys, points, num_points, evals, num_evals, tr,
      [&](const Fr* g_prime, const HFr* point) { ipa_open(c, p, poly_size, g_prime, num_vars, point, tr); }, small);
}

Pcs ipa_pcs(Ctx& c, const IpaParams& p, size_t poly_size) {
  Pcs pcs;
  pcs.max_vars = ipa_trim_vars(p, poly_size);
  const G1Affine* g = device_g(p);
  pcs.batch_commit = [&c, &p, poly_size](const Fr* const* polys, size_t np, size_t nv) {
    return ipa_batch_commit(c, p, poly_size, polys, np, nv);
  };
  pcs.commit_bases = [g](size_t) { return g; };  // a prefix of g commits a zero-padded table
  pcs.batch_open = [&c, &p, poly_size](size_t nv, const Fr* const* polys, size_t np, const HFr* points, size_t npts,
                                       const lh_evaluation* evals, size_t ne, Transcript& tr, const SmallPoly* small) {
    ipa_batch_open(c, p, poly_size, nv, polys, np, points, npts, evals, ne, tr, small);
  };
  return pcs;
}

// ------------------------------------------------------------------ Hyrax (hyrax.rs:121-271)
HyraxDims hyrax_dims(size_t poly_size, size_t batch_size) {
  HyraxDims d;
  d.num_vars = log2_exact(poly_size, "hyrax");
  LH_REQUIRE(batch_size > 0 && batch_size <= poly_size, LH_ERR_ARG, "hyrax: batch_size must be in 1..poly_size");  // hyrax.rs:123
  LH_REQUIRE(d.num_vars >= 1 && d.num_vars <= 32, LH_ERR_ARG, "hyrax: num_vars must be in 1..32");
  while (((size_t)1 << d.batch_num_vars) < poly_size * batch_size) d.batch_num_vars++;  // next_power_of_two().ilog2()
  d.row_num_vars = (d.batch_num_vars + 1) / 2;
  return d;
}
HyraxDims hyrax_trim(const IpaParams& p, size_t poly_size, size_t batch_size) {
  const HyraxDims d = hyrax_dims(poly_size, batch_size);
  if (p.num_vars < d.row_num_vars)
    throw Error(LH_ERR_INVALID_PCS_PARAM, "Too many variates to trim (param supports variates up to " +
                                              std::to_string(p.num_vars) + " but got " + std::to_string(d.row_num_vars) + ")");
  return d;
}

// the window table of g[0 .. row_len) the row kernels file their terms from (dev.hpp k_g1_rows_msm): 32 windows of 8 bits,
// row_len * 2 KiB - 8 MiB at the 4096 columns of a 2^24-entry table; built on first use by the ctx that asks, kept on the param.
// One entry per distinct row_len (i.e. per trim / batch size used with the param), never evicted before ipa_free: a handful of
// tables of a few MiB today.  The param's mutex is held while a table is built (a hipMalloc, one kernel, a sync): a second
// caller needs that very table, and nothing else of the param is touched while a commit runs.
constexpr uint32_t HYRAX_ROWS_CBITS = 8, HYRAX_ROWS_W = 32;
const G1Affine* ipa_rows_table(Ctx& c, const IpaParams& p, size_t row_len) {
  const G1Affine* g = device_g(p);
  // (the table is built by this ctx's stream and lives beside g: both on the param's device)
  LH_REQUIRE(c.device == p.d_g.device(), LH_ERR_ARG, "hyrax commit: the ctx and the param's bases are on different devices");
  OnDevice on(c.device);
  std::lock_guard<std::mutex> lk(p.mu);
  auto it = p.rows_tables.find(row_len);
  if (it != p.rows_tables.end()) return it->second;
  DevMem t(row_len * HYRAX_ROWS_W * sizeof(G1Affine));
  k_msm_window_table(c, g, row_len, HYRAX_ROWS_CBITS, HYRAX_ROWS_W, t);
  c.sync();
  return p.rows_tables[row_len] = std::move(t);
}

// Options::hyrax_rows 1: every row of every poly in ONE call of the row kernels (kernels_hyrax.hip); 0: every row a job of
// ONE msm_batch over g (msm_batch itself plans 48 jobs at a time).  The same points either way.
std::vector<HG1> hyrax_batch_commit(Ctx& c, const IpaParams& p, size_t poly_size, size_t batch_size, const Fr* const* d_polys,
                                    size_t num_polys, size_t num_vars) {
  const HyraxDims d = hyrax_trim(p, poly_size, batch_size);
  check_vars(d.num_vars, num_vars, num_polys == 1 ? "commit" : "batch commit");
  // (the reference cuts a smaller poly into fewer rows and then groups them by the PARAM's row count: only equal sizes work)
  LH_REQUIRE(num_vars == d.num_vars, LH_ERR_ARG, "hyrax commit: the poly must have as many variables as the (trimmed) param");
  const size_t chunks = d.num_chunks(), row_len = (size_t)1 << d.row_num_vars;
  std::vector<HG1> out(num_polys * chunks);
  if (!num_polys) return out;
  const G1Affine* g = device_g(p);
  if (c.opt.hyrax_rows) {
    std::vector<RowsMsmCol> cols(num_polys);
    for (size_t i = 0; i < num_polys; i++) cols[i] = RowsMsmCol{d_polys[i], false, 0, chunks * row_len};
    k_g1_rows_msm_batch(c, cols.data(), num_polys, chunks, row_len, g, ipa_rows_table(c, p, row_len), HYRAX_ROWS_CBITS, HYRAX_ROWS_W,
                        (G1Affine*)out.data());
    return out;
  }
  std::vector<MsmJob> jobs;
  jobs.reserve(out.size());
  for (size_t i = 0; i < num_polys; i++)
    for (size_t r = 0; r < chunks; r++) jobs.push_back(MsmJob{d_polys[i] + r * row_len, false, g, row_len});
  msm_batch(c, jobs.data(), jobs.size(), (G1Affine*)out.data());
  return out;
}

void hyrax_open(Ctx& c, const IpaParams& p, size_t poly_size, size_t batch_size, const Fr* d_poly, size_t num_vars,
                const HFr* point, Transcript& tr) {
  const HyraxDims d = hyrax_trim(p, poly_size, batch_size);
  check_vars(d.num_vars, num_vars, "open");
  LH_REQUIRE(num_vars == d.num_vars, LH_ERR_ARG, "hyrax open: the poly must have as many variables as the (trimmed) param");
  const size_t chunks = d.num_chunks(), row_len = (size_t)1 << d.row_num_vars;
  ArenaScope scope(c.arena);
  const Fr* row = d_poly;  // hi empty: the poly is its single row (hyrax.rs:240-244)
  if (chunks > 1) {
    const size_t hi_vars = num_vars - d.row_num_vars;
    std::vector<Fr> hi(hi_vars);
    for (size_t i = 0; i < hi_vars; i++) hi[i] = dev(point[d.row_num_vars + i]);
    Fr* w = c.arena.alloc_n<Fr>(chunks);
    Fr* combined = c.arena.alloc_n<Fr>(row_len);
    k_eq_xy(c, hi.data(), hi_vars, w);
    k_hyrax_combine(c, d_poly, w, chunks, row_len, combined);  // fix_last_vars(hi)
    row = combined;
  }
  ipa_open(c, p, row_len, row, d.row_num_vars, point, tr);
}

void hyrax_batch_open(Ctx& c, const IpaParams& p, size_t poly_size, size_t batch_size, size_t num_vars, const Fr* const* d_polys,
                      size_t num_polys, const HFr* points, size_t num_points, const lh_evaluation* evals, size_t num_evals,
                      Transcript& tr, const SmallPoly* small) {
  const HyraxDims d = hyrax_trim(p, poly_size, batch_size);
  check_vars(d.num_vars, num_vars, "open");
  additive_batch_open(
      c, num_vars, d_polys, num_polys, points, num_points, evals, num_evals, tr,
      [&](const Fr* g_prime, const HFr* point) { hyrax_open(c, p, poly_size, batch_size, g_prime, num_vars, point, tr); }, small);
}

// columns of at most 2^num_vars entries, zero-padded: rows beyond a column's length are identities and cost nothing
static std::vector<HG1> hyrax_commit_columns(Ctx& c, const IpaParams& p, const HyraxDims& d, const PcsColumn* cols, size_t num_cols,
                                             size_t nv) {
  LH_REQUIRE(nv == d.num_vars, LH_ERR_ARG, "hyrax commit: the poly must have as many variables as the (trimmed) param");
  const size_t chunks = d.num_chunks(), row_len = (size_t)1 << d.row_num_vars;
  std::vector<HG1> out(num_cols * chunks, HG1{host::Fq::zero(), host::Fq::zero()});
  if (!num_cols) return out;
  const G1Affine* g = device_g(p);
  for (size_t i = 0; i < num_cols; i++) LH_REQUIRE(cols[i].len <= chunks * row_len, LH_ERR_ARG, "hyrax commit: a column is longer than the table");
  if (c.opt.hyrax_rows) {
    std::vector<RowsMsmCol> rc(num_cols);
    for (size_t i = 0; i < num_cols; i++) rc[i] = RowsMsmCol{cols[i].data, cols[i].u32, cols[i].known_bits, cols[i].len};
    k_g1_rows_msm_batch(c, rc.data(), num_cols, chunks, row_len, g, ipa_rows_table(c, p, row_len), HYRAX_ROWS_CBITS, HYRAX_ROWS_W,
                        (G1Affine*)out.data());
    return out;
  }
  std::vector<MsmJob> jobs;
  std::vector<size_t> slot;
  for (size_t i = 0; i < num_cols; i++)
    for (size_t r = 0; r * row_len < cols[i].len; r++) {
      const size_t first = r * row_len;
      MsmJob jb{(const char*)cols[i].data + first * (cols[i].u32 ? 4 : 32), cols[i].u32, g, std::min(row_len, cols[i].len - first)};
      jb.known_bits = cols[i].u32 ? cols[i].known_bits : 0;
      jobs.push_back(jb), slot.push_back(i * chunks + r);
    }
  std::vector<HG1> part(jobs.size());
  if (!jobs.empty()) msm_batch(c, jobs.data(), jobs.size(), (G1Affine*)part.data());
  for (size_t k = 0; k < jobs.size(); k++) out[slot[k]] = part[k];
  return out;
}

Pcs hyrax_pcs(Ctx& c, const IpaParams& p, size_t poly_size, size_t batch_size) {
  const HyraxDims d = hyrax_trim(p, poly_size, batch_size);
  device_g(p);
  Pcs pcs;
  pcs.max_vars = d.num_vars;
  pcs.chunks = d.num_chunks();
  pcs.batch_commit = [&c, &p, poly_size, batch_size](const Fr* const* polys, size_t np, size_t nv) {
    return hyrax_batch_commit(c, p, poly_size, batch_size, polys, np, nv);
  };
  pcs.commit_columns = [&c, &p, d](const PcsColumn* cols, size_t nc, size_t nv) { return hyrax_commit_columns(c, p, d, cols, nc, nv); };
  pcs.batch_open = [&c, &p, poly_size, batch_size](size_t nv, const Fr* const* polys, size_t np, const HFr* points, size_t npts,
                                                   const lh_evaluation* evals, size_t ne, Transcript& tr, const SmallPoly* small) {
    hyrax_batch_open(c, p, poly_size, batch_size, nv, polys, np, points, npts, evals, ne, tr, small);
  };
  return pcs;
}

}  // namespace lh
