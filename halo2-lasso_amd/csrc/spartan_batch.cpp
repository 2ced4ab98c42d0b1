// Batched Spartan, the verifier: K' >= 2 assignments of ONE R1CS key (spartan.cpp) in one proof.  The assignments are
// stacked instance-minor - Z[i + K y], K = 2^k >= K', the instance in the low k coordinates, the instances beyond K' zero -;
// the outer sum-check runs over k + l variables and brings every instance to one r_x = r[k ..), so ONE inner sum-check over
// the eq(r_b, .)-weighted combination of the assignments, ONE opening of the stacked witness and ONE set of three Spark
// openings finish it.  Host only.  The reference holds no such argument; protocol and transcript schedule are specified in
// tests/spartan_batch_ref.py, whose proofs (tests/golden/spartan_batch.json) this verifier accepts.  Written against the PCS
// description (host.hpp PcsVerifier), the arguments' shared steps (argument.cpp) and the verifier's steps of spartan.cpp.
#include <algorithm>
#include "host.hpp"

namespace lh {

namespace {
// step 0: the key part, K', the public inputs instance by instance
void batch_header(Transcript& tr, size_t n, size_t l, size_t p, const std::vector<HG1>* comms, const HFr* x, size_t count) {
  spartan_key_header(tr, n, l, p, comms);
  tr.common_field_element(HFr::from_u64(count));
  for (size_t i = 0; i < count * p; i++) tr.common_field_element(x[i]);
}

void verify_batch_checked(const PcsVerifier& pcs, size_t n, size_t l, size_t k, const uint8_t* key, size_t key_len, const HFr* x,
                          size_t count, size_t p, Transcript& tr) {
  const SpartanKeyBlob kb = spartan_read_key("spartan", key, key_len);
  batch_header(tr, n, l, p, kb.comms, x, count);
  const std::vector<HG1> cw = lasso_read_commitments(tr, 1);
  const std::vector<HFr> tau = tr.squeeze_challenges(k + l);
  const std::pair<HFr, std::vector<HFr>> outer = sum_check_verify(LH_SC_EVALUATIONS, k + l, 3, HFr::zero(), tr);
  const std::vector<HFr>& r = outer.second;
  const std::vector<HFr> v = tr.read_field_elements(3);
  if (outer.first != host_eq_xy_eval(tau.data(), r.data(), k + l) * (v[0] * v[1] - v[2]))
    throw Error(LH_ERR_INVALID_SNARK, "spartan: outer sum-check final evaluation mismatch");
  const std::vector<HFr> r_x(r.begin() + k, r.end());
  const SpartanInnerClaim claim = spartan_inner_rounds_verify(l, v.data(), tr);
  // xbar[j] = sum_{i < K'} eq(r_b, i) x_i[j]: K' p products, and k per weight
  std::vector<HFr> xbar(p, HFr::zero());
  for (size_t i = 0; i < count; i++) {
    HFr w = HFr::one();
    for (size_t b = 0; b < k; b++) w = w * ((i >> b) & 1 ? r[b] : HFr::one() - r[b]);
    for (size_t j = 0; j < p; j++) xbar[j] = xbar[j] + w * x[i * p + j];
  }
  std::vector<HFr> point(r.begin(), r.begin() + k);
  point.insert(point.end(), claim.r_y.begin(), claim.r_y.end() - 1);
  spartan_witness_verify(pcs, claim, l, xbar.data(), p, cw[0], k + l - 1, point.data(), tr);
  spartan_verify_matrices(pcs, n, l, kb, r_x, claim.r_y, claim.e, tr);
}
}  // namespace

size_t spartan_batch_check(size_t l, size_t count) {
  LH_REQUIRE(count >= 2, LH_ERR_ARG, "spartan: num_instances out of range (at least 2)");
  size_t k = 1;
  while (((size_t)1 << k) < count && k < 63) k++;
  LH_REQUIRE(l + k <= (size_t)LH_SPARTAN_BATCH_MAX_VARS, LH_ERR_ARG,
             "spartan: dim_vars + batch_vars out of range (at most " + std::to_string(LH_SPARTAN_BATCH_MAX_VARS) + ")");
  return k;
}

void spartan_verify_batch(const PcsVerifier& pcs, size_t n, size_t l, const uint8_t* key, size_t key_len, const HFr* x, size_t count,
                          size_t p, Transcript& tr) {
  spartan_check(n, l, p);
  const size_t k = spartan_batch_check(l, count);
  LH_REQUIRE(key != nullptr && x != nullptr, LH_ERR_ARG, "null argument: key or x");
  argument_pcs_check(pcs, "spartan");
  try {
    argument_verdict("spartan", [&] { verify_batch_checked(pcs, n, l, k, key, key_len, x, count, p, tr); });
  } catch (const Error& e) {  // (a piece that gives its verdict itself: under this argument's name too, as spartan_verify)
    if (e.code != LH_ERR_INVALID_SNARK || e.msg.rfind("spartan: ", 0) == 0) throw;
    throw Error(LH_ERR_INVALID_SNARK, "spartan: " + e.msg);
  }
}

}  // namespace lh
