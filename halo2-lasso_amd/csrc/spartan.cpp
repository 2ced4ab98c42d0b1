// Spartan (Setty, CRYPTO 2020) over the Spark-committed matrices of an R1CS: (Az)[i] (Bz)[i] = (Cz)[i] for every row, with
// z = (w, x, 0).  The outer sum-check reduces the 2^l row identities to three values of Az, Bz, Cz at r_x; the inner one
// reduces those to A~, B~, C~ at (r_x, r_y) and z~(r_y); the witness is opened, the matrices are opened by Spark against
// the key.  Both matrix products - M z by rows and the matrix bound at r_x by columns - are the keyed field sum of
// kernels_spartan.hip over the sorted entry streams the key holds.  The reference holds no such argument; protocol and
// transcript schedule are specified in tests/spartan_ref.py and reproduced here byte for byte.  Written against the PCS
// description (host.hpp Pcs / PcsVerifier) and the arguments' shared steps (argument.cpp), as spark.cpp is.
#include <algorithm>
#include "host.hpp"

namespace lh {

namespace {
constexpr size_t SPARTAN_COMMITTED = 1 + 3 * 2;  // the polys of a matrix's Spark commitment (c = 2)

// step 0: the key part (spartan_key_header), then x
void spartan_header(Transcript& tr, size_t n, size_t l, size_t p, const std::vector<HG1>* comms, const HFr* x) {
  spartan_key_header(tr, n, l, p, comms);
  for (size_t i = 0; i < p; i++) tr.common_field_element(x[i]);
}

lh_sop outer_expression() {  // eq(tau, .) (Poly0 Poly1 - Poly2)
  lh_sop sop;
  memset(&sop, 0, sizeof(sop));
  sop.num_terms = 2, sop.global_eq = 0;
  const HFr one = HFr::one(), minus = HFr::zero() - HFr::one();
  memcpy(&sop.coeff[0], &one, 32), memcpy(&sop.coeff[1], &minus, 32);
  sop.num_factors[0] = 2, sop.factor[0][0] = 0, sop.factor[0][1] = 1;
  sop.num_factors[1] = 1, sop.factor[1][0] = 2;
  return sop;
}
lh_sop inner_expression(const HFr& rho) {  // (M_A + rho M_B + rho^2 M_C) z over [M_A, M_B, M_C, z]
  lh_sop sop;
  memset(&sop, 0, sizeof(sop));
  sop.num_terms = 3, sop.global_eq = -1;
  HFr w = HFr::one();
  for (size_t m = 0; m < 3; m++, w = w * rho) {
    memcpy(&sop.coeff[m], &w, 32);
    sop.num_factors[m] = 2, sop.factor[m][0] = (uint8_t)m, sop.factor[m][1] = 3;
  }
  return sop;
}
}  // namespace

void spartan_key_header(Transcript& tr, size_t n, size_t l, size_t p, const std::vector<HG1>* comms) {
  for (size_t v : {n, l, p}) tr.common_field_element(HFr::from_u64(v));
  for (size_t m = 0; m < 3; m++) argument_absorb_commitments(tr, comms[m]);
}
std::vector<lh_evaluation> spartan_doubled_evaluation(const HFr& e) { return {make_evaluation(0, 0, &e), make_evaluation(0, 0, &e)}; }

void spartan_spmv(Ctx& c, const R1csKey& key, int direction, const Fr* X, Fr* const* out) {
  SpartanSpmv a;
  memset(&a, 0, sizeof(a));
  for (size_t m = 0; m < 3; m++) {
    a.seg[m] = key.seg[direction][m], a.other[m] = key.other[direction][m], a.perm[m] = key.perm[direction][m];
    a.val[m] = key.mat[m]->val, a.out[m] = out[m];
  }
  a.X = X;
  k_spartan_spmv(c, a, (size_t)1 << key.n, key.l);
}
void spartan_require_key(Ctx& c, const R1csKey& key, const char* name) {
  LH_REQUIRE(std::find(c.r1cs_keys.begin(), c.r1cs_keys.end(), &key) != c.r1cs_keys.end(), LH_ERR_ARG,
             std::string(name) + ": the key was not committed on this ctx (or has been freed)");
}
void spartan_assignment(Ctx& c, size_t l, const Fr* d_w, const HFr* x, size_t p, Fr* z) {
  const size_t half = (size_t)1 << (l - 1);
  LH_HIP(hipMemcpyAsync(z, d_w, half * sizeof(Fr), hipMemcpyDeviceToDevice, c.stream));
  LH_HIP(hipMemcpyAsync(z + half, x, p * sizeof(Fr), hipMemcpyHostToDevice, c.stream));
  if (p < half) LH_HIP(hipMemsetAsync(z + half + p, 0, (half - p) * sizeof(Fr), c.stream));
}

size_t spartan_check(size_t n, size_t l, size_t p) {
  LH_REQUIRE(l >= (size_t)LH_SPARTAN_MIN_DIM_VARS && l <= (size_t)LH_SPARTAN_MAX_DIM_VARS, LH_ERR_ARG,
             "spartan: dim_vars out of range (" + std::to_string(LH_SPARTAN_MIN_DIM_VARS) + " to " +
                 std::to_string(LH_SPARTAN_MAX_DIM_VARS) + ")");
  LH_REQUIRE(n >= 1 && n < 31, LH_ERR_ARG, "spartan: num_vars out of range (1 to 30)");  // (Spark's)
  LH_REQUIRE(p >= 1 && p <= (size_t)1 << (l - 1), LH_ERR_ARG, "spartan: num_public out of range (1 to 2^(dim_vars - 1))");
  return std::max(n, l);
}

void spartan_free(Ctx& c, R1csKey* key) {
  auto it = std::find(c.r1cs_keys.begin(), c.r1cs_keys.end(), key);
  if (it == c.r1cs_keys.end()) return;
  c.r1cs_keys.erase(it);
  (void)hipStreamSynchronize(c.stream);  // (a prove queued on the stream may still read the streams)
  delete key;
}
R1csKey::~R1csKey() {
  for (SparkPoly* p : mat)
    if (p) spark_free(*ctx, p);
}
void spartan_free_all(Ctx& c) {
  while (!c.r1cs_keys.empty()) spartan_free(c, c.r1cs_keys.back());
}

R1csKey* spartan_commit(Ctx& c, const Pcs& pcs, size_t n, size_t l, const lh_r1cs_matrix* m) {
  const size_t nv = spartan_check(n, l, 1);
  LH_REQUIRE(m != nullptr, LH_ERR_ARG, "null argument: m");
  for (size_t i = 0; i < 3; i++)
    LH_REQUIRE(m[i].d_row && m[i].d_col && m[i].d_val, LH_ERR_ARG, "null argument: a column of m[" + std::to_string(i) + "]");
  argument_not_sharded(c, "spartan");
  argument_pcs_check(pcs, nv, "spartan", true);
  const size_t N = (size_t)1 << n;
  std::unique_ptr<R1csKey> owner(new R1csKey());
  R1csKey& key = *owner;
  key.ctx = &c, key.n = n, key.l = l;
  // (a refusal below - an index out of range in B, say - gives back what was made: the key's destructor)
  // ---- the three Spark commitments, in the caller's entry order: what three separate spark_commit calls give
  for (size_t i = 0; i < 3; i++) {
    const uint32_t* dims[2] = {m[i].d_row, m[i].d_col};
    key.mat[i] = spark_commit(c, pcs, n, l, 2, dims, (const Fr*)m[i].d_val);
    key.blob.insert(key.blob.end(), key.mat[i]->blob.begin(), key.mat[i]->blob.end());
  }
  // ---- the sorted streams: per matrix and direction two stable sorts of the handle's (checked) copies by the same key -
  // one carries the other index along, one the positions - all twelve as ONE launch set per radix pass
  key.block.alloc(18 * N * sizeof(uint32_t));
  {
    ArenaScope scope(c.arena);
    uint32_t* words = key.block.as<uint32_t>();
    uint32_t* again = c.arena.alloc_n<uint32_t>(6 * N);  // (the second sorts' keys: the first ones' once more)
    std::vector<SortSlab> slabs;
    for (int d = 0; d < 2; d++)
      for (size_t i = 0; i < 3; i++) {
        uint32_t* at = words + (d * 3 + i) * 3 * N;
        key.seg[d][i] = at, key.other[d][i] = at + N, key.perm[d][i] = at + 2 * N;
        const uint32_t *by = key.mat[i]->dim[d], *along = key.mat[i]->dim[1 - d];
        slabs.push_back(SortSlab{by, at, along, at + N, N, (unsigned)l});
        slabs.push_back(SortSlab{by, again + (d * 3 + i) * N, nullptr, at + 2 * N, N, (unsigned)l});
      }
    // (launch record "spartan_key_sort": twelve slabs of N pairs, read and written once - the passes are the sort's business)
    ProfScope ps(c, "spartan_key_sort", 12.0 * 16.0 * N, 0.0, 12.0 * N);
    sort_pairs_u32_batched(c, slabs.data(), slabs.size());
    c.sync();
  }
  c.r1cs_keys.push_back(&key);
  return owner.release();
}

void spartan_debug_spmv(Ctx& c, const R1csKey& key, int direction, const Fr* d_x, Fr* const* d_out) {
  spartan_require_key(c, key, "spartan");
  LH_REQUIRE(direction == 0 || direction == 1, LH_ERR_ARG, "spartan: direction is 0 (by rows) or 1 (by columns)");
  LH_REQUIRE(d_x && d_out && d_out[0] && d_out[1] && d_out[2], LH_ERR_ARG, "null argument: d_x or d_out");
  spartan_spmv(c, key, direction, d_x, d_out);
  c.sync();
}

void spartan_prove(Ctx& c, const Pcs& pcs, const R1csKey& key, const Fr* d_w, const HFr* x, size_t p, Transcript& tr) {
  spartan_require_key(c, key, "spartan");
  const size_t n = key.n, l = key.l;
  const size_t nv = spartan_check(n, l, p);
  LH_REQUIRE(d_w != nullptr && x != nullptr, LH_ERR_ARG, "null argument: d_w or x");
  argument_not_sharded(c, "spartan");
  argument_pcs_check(pcs, nv, "spartan", true);
  const size_t M = (size_t)1 << l;
  open_precommit_cancel(c);
  std::vector<HFr> r_x, r_y, e;
  {
    ArenaScope scope(c.arena);
    EqHalfScope eq_scope(c);
    // ---- 3 first: z = (w, x, 0), Az, Bz, Cz and the satisfaction count need no challenge - a witness that does not
    // satisfy the instance is refused before the transcript is touched
    Fr* z = c.arena.alloc_n<Fr>(M);
    spartan_assignment(c, l, d_w, x, p, z);
    Fr* Mz[3];
    for (Fr*& t : Mz) t = c.arena.alloc_n<Fr>(M);
    spartan_spmv(c, key, 0, z, Mz);
    const size_t bad = k_spartan_unsatisfied(c, Mz[0], Mz[1], Mz[2], M);
    LH_REQUIRE(bad == 0, LH_ERR_ARG,
               "spartan: the witness does not satisfy " + std::to_string(bad) + " of the 2^" + std::to_string(l) + " constraints");

    // ---- 0/1/2: header; the commitment of w; tau
    std::vector<HG1> comms[3];
    for (size_t m = 0; m < 3; m++) comms[m] = key.mat[m]->comms;
    spartan_header(tr, n, l, p, comms, x);
    lasso_write_commitments(tr, pcs.batch_commit(&d_w, 1, l - 1));
    const std::vector<HFr> tau = tr.squeeze_challenges(l);

    // ---- 4: the outer sum-check, claim 0 (exact: the count above), then Az, Bz, Cz at r_x
    ScOptions so;
    so.sum_is_exact = true;
    std::vector<HFr> at_rx;
    {
      const Fr* polys[3] = {Mz[0], Mz[1], Mz[2]};
      SumCheckResult sc = sum_check_prove(c, LH_SC_EVALUATIONS, l, outer_expression(), polys, 3, tau.data(), 1, HFr::zero(), tr, so);
      r_x = sc.challenges, at_rx = sc.evals;
    }
    tr.write_field_elements(at_rx);

    // ---- 5 to 8: the inner half
    spartan_inner_prove(c, pcs, key, z, d_w, Mz, r_x, at_rx.data(), tr, r_y, e);
  }
  // ---- 9: the three Spark openings at r_x || r_y, on the same transcript
  spartan_open_matrices(c, pcs, key, r_x, r_y, e, tr);
}

// steps 5 to 8, from rho to the opening of w: what the plain and the relaxed prover share.  Mz: the three tables of step 3,
// done with - they take the matrices bound at r_x
void spartan_inner_prove(Ctx& c, const Pcs& pcs, const R1csKey& key, const Fr* z, const Fr* d_w, Fr* const* Mz,
                         const std::vector<HFr>& r_x, const HFr* at_rx, Transcript& tr, std::vector<HFr>& r_y, std::vector<HFr>& e) {
  const size_t l = key.l, M = (size_t)1 << l;
  ScOptions so;
  so.sum_is_exact = true;
  e.resize(3);
  // ---- 5/6/7: rho; the matrices bound at r_x (the same keyed sum by columns, over the eq table of r_x; the tables of
  // step 3 are done with and take the result); the inner sum-check, then the values at r_y
  const HFr rho = tr.squeeze_challenge();
  const HFr T = at_rx[0] + rho * at_rx[1] + rho * rho * at_rx[2];
  {
    ArenaScope inner(c.arena);
    Fr* eq_rx = c.arena.alloc_n<Fr>(M);
    k_eq_xy(c, (const Fr*)r_x.data(), l, eq_rx);
    spartan_spmv(c, key, 1, eq_rx, Mz);
  }
  {
    const Fr* polys[4] = {Mz[0], Mz[1], Mz[2], z};
    SumCheckResult sc = sum_check_prove(c, LH_SC_EVALUATIONS, l, inner_expression(rho), polys, 4, nullptr, 0, T, tr, so);
    r_y = sc.challenges;
    std::copy(sc.evals.begin(), sc.evals.begin() + 3, e.begin());
  }
  tr.write_field_elements(e);
  const HFr e_w = evaluate_polys(c, &d_w, 1, l - 1, r_y.data())[0];
  tr.write_field_element(e_w);

  // ---- 8: the opening of w at r_y[0 .. l-1)
  const std::vector<lh_evaluation> evs = spartan_doubled_evaluation(e_w);
  pcs.batch_open(l - 1, &d_w, 1, r_y.data(), 1, evs.data(), evs.size(), tr, nullptr);
}
void spartan_open_matrices(Ctx& c, const Pcs& pcs, const R1csKey& key, const std::vector<HFr>& r_x, const std::vector<HFr>& r_y,
                           const std::vector<HFr>& e, Transcript& tr) {
  std::vector<HFr> point(r_x);
  point.insert(point.end(), r_y.begin(), r_y.end());
  for (size_t m = 0; m < 3; m++) {
    const HFr v = spark_open(c, pcs, *key.mat[m], point.data(), tr);
    LH_REQUIRE(v == e[m], LH_ERR_DEVICE, "spartan: a matrix's Spark value differs from the inner sum-check's");
  }
}

SpartanKeyBlob spartan_read_key(const char* name, const uint8_t* key, size_t key_len) {
  const std::string malformed = std::string(name) + ": malformed key: ";
  SpartanKeyBlob k;
  const uint8_t** blob = k.blob;
  size_t* blob_len = k.blob_len;
  std::vector<HG1>* comms = k.comms;
  // the key blob: three commitment blobs, each its mask element and its non-identity points
  size_t at = 0;
  for (size_t m = 0; m < 3; m++) {
    if (key_len < at + 32) throw Error(LH_ERR_INVALID_SNARK, malformed + "too short");
    size_t absent = 0;
    for (size_t i = 0; i < 32; i++) absent += (size_t)__builtin_popcount(key[at + i]);
    // (a mask out of range is refused by the reader below; here it must only not run the length negative)
    const size_t len = 32 + 64 * (SPARTAN_COMMITTED - std::min(absent, SPARTAN_COMMITTED));
    if (key_len < at + len) throw Error(LH_ERR_INVALID_SNARK, malformed + "too short");
    blob[m] = key + at, blob_len[m] = len;
    comms[m] = argument_read_commitment_blob(name, blob[m], len, SPARTAN_COMMITTED);
    at += len;
  }
  if (at != key_len) throw Error(LH_ERR_INVALID_SNARK, malformed + "wrong length");
  return k;
}
// the verifier's steps 5 to 8, from rho to the opening of w (cw: its commitment; v: vA, vB, vC) -> r_y and eA, eB, eC: its two
// halves in their order
void spartan_inner_verify(const PcsVerifier& pcs, size_t l, const HFr* x, size_t p, const HG1& cw, const HFr* v, Transcript& tr,
                          std::vector<HFr>& r_y, std::vector<HFr>& e) {
  const SpartanInnerClaim claim = spartan_inner_rounds_verify(l, v, tr);
  r_y = claim.r_y, e = claim.e;
  spartan_witness_verify(pcs, claim, l, x, p, cw, l - 1, r_y.data(), tr);
}
SpartanInnerClaim spartan_inner_rounds_verify(size_t l, const HFr* v, Transcript& tr) {
  SpartanInnerClaim claim;
  claim.rho = tr.squeeze_challenge();
  const HFr& rho = claim.rho;
  const std::pair<HFr, std::vector<HFr>> inner = sum_check_verify(LH_SC_EVALUATIONS, l, 2, v[0] + rho * v[1] + rho * rho * v[2], tr);
  claim.final = inner.first, claim.r_y = inner.second;
  claim.e = tr.read_field_elements(3);
  return claim;
}
// e_w, the inner final claim over z~(r_y) = (1 - r_y[l-1]) e_w + r_y[l-1] x~(r_y[0 .. l-1)), the opening of the witness of
// `vars` variables at `point` (the batch verifier's: the stacked witness, at r_b || r_y[0 .. l-1))
void spartan_witness_verify(const PcsVerifier& pcs, const SpartanInnerClaim& claim, size_t l, const HFr* x, size_t p, const HG1& cw,
                            size_t vars, const HFr* point, Transcript& tr) {
  const std::vector<HFr>&r_y = claim.r_y, &e = claim.e;
  const HFr& rho = claim.rho;
  const HFr e_w = tr.read_field_element();
  // z~(r_y): the public half at a cost that follows p - x padded to 2^q, the first q coordinates, the rest of the half's
  // coordinates at their zero side
  size_t q = 0;
  while (((size_t)1 << q) < p) q++;
  HFr x_ry = q == 0 ? x[0] : host_table_eval(q, r_y, [&](size_t i) { return i < p ? x[i] : HFr::zero(); });
  for (size_t i = q; i + 1 < l; i++) x_ry = x_ry * (HFr::one() - r_y[i]);
  const HFr z_ry = (HFr::one() - r_y[l - 1]) * e_w + r_y[l - 1] * x_ry;
  if (claim.final != (e[0] + rho * e[1] + rho * rho * e[2]) * z_ry)
    throw Error(LH_ERR_INVALID_SNARK, "spartan: inner sum-check final evaluation mismatch");
  const std::vector<lh_evaluation> evs = spartan_doubled_evaluation(e_w);
  pcs.batch_verify(vars, &cw, 1, point, 1, evs.data(), evs.size(), tr);
}
void spartan_verify_matrices(const PcsVerifier& pcs, size_t n, size_t l, const SpartanKeyBlob& k, const std::vector<HFr>& r_x,
                             const std::vector<HFr>& r_y, const std::vector<HFr>& e, Transcript& tr) {
  std::vector<HFr> point(r_x);
  point.insert(point.end(), r_y.begin(), r_y.end());
  for (size_t m = 0; m < 3; m++) {
    try {
      spark_verify(pcs, n, l, 2, k.blob[m], k.blob_len[m], point.data(), e[m], tr);
    } catch (const Error& err) {
      if (err.code != LH_ERR_INVALID_SNARK) throw;
      throw Error(LH_ERR_INVALID_SNARK, std::string("spartan: matrix ") + "ABC"[m] + ": " + err.msg);
    }
  }
}

static void spartan_verify_checked(const PcsVerifier& pcs, size_t n, size_t l, const uint8_t* key, size_t key_len, const HFr* x,
                                   size_t p, Transcript& tr) {
  const SpartanKeyBlob k = spartan_read_key("spartan", key, key_len);
  const std::vector<HG1>* comms = k.comms;
  spartan_header(tr, n, l, p, comms, x);
  const std::vector<HG1> cw = lasso_read_commitments(tr, 1);
  const std::vector<HFr> tau = tr.squeeze_challenges(l);
  const std::pair<HFr, std::vector<HFr>> outer = sum_check_verify(LH_SC_EVALUATIONS, l, 3, HFr::zero(), tr);
  const std::vector<HFr>& r_x = outer.second;
  const std::vector<HFr> v = tr.read_field_elements(3);
  if (outer.first != host_eq_xy_eval(tau.data(), r_x.data(), l) * (v[0] * v[1] - v[2]))
    throw Error(LH_ERR_INVALID_SNARK, "spartan: outer sum-check final evaluation mismatch");
  std::vector<HFr> r_y, e;
  spartan_inner_verify(pcs, l, x, p, cw[0], v.data(), tr, r_y, e);
  spartan_verify_matrices(pcs, n, l, k, r_x, r_y, e, tr);
}
void spartan_verify(const PcsVerifier& pcs, size_t n, size_t l, const uint8_t* key, size_t key_len, const HFr* x, size_t p,
                    Transcript& tr) {
  spartan_check(n, l, p);
  LH_REQUIRE(key != nullptr && x != nullptr, LH_ERR_ARG, "null argument: key or x");
  argument_pcs_check(pcs, "spartan");
  try {
    argument_verdict("spartan", [&] { spartan_verify_checked(pcs, n, l, key, key_len, x, p, tr); });
  } catch (const Error& e) {  // (a piece that gives its verdict itself - a commitment block's mask -: under this argument's name too)
    if (e.code != LH_ERR_INVALID_SNARK || e.msg.rfind("spartan: ", 0) == 0) throw;
    throw Error(LH_ERR_INVALID_SNARK, "spartan: " + e.msg);
  }
}

}  // namespace lh
