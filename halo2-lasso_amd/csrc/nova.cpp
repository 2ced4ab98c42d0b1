// Nova folding (Kothapalli, Setty, Tzialla, CRYPTO 2022) for the R1CS keys of spartan.cpp, and the relaxed form of Spartan
// that closes a chain of folds.  A relaxed instance is (C_W, C_E, x) with u = x[0]: (Az)[i] (Bz)[i] = u (Cz)[i] + E[i] for
// every row, z = (w, x, 0).  A fold is the six products M z by ONE keyed sum with two right-hand sides over the key's sorted
// streams (kernels_nova.hip), one pass for the cross term T and the rows that fail, one commitment, one linear combination;
// the commitments fold on the host.  The reference holds no such argument; protocol and transcript schedule are specified in
// tests/nova_ref.py and reproduced here byte for byte.  Written against the PCS description (host.hpp Pcs / PcsVerifier),
// the arguments' shared steps (argument.cpp) and the steps of spartan.cpp.
#include <algorithm>
#include "host.hpp"

namespace lh {

namespace {
struct NovaInstance {
  HG1 cw, ce;
  std::vector<HFr> x;
};

// the bytes of an instance: a transcript's stream of its own
std::vector<uint8_t> instance_blob(const NovaInstance& U) {
  KeccakTranscript kt;
  Transcript tr(&kt.vt);
  lasso_write_commitments(tr, {U.cw, U.ce});
  tr.write_field_elements(U.x);
  return kt.stream;
}
// the number of public inputs of a blob, from its mask and its length
size_t instance_num_public(const std::string& malformed, int code, const uint8_t* blob, size_t len) {
  if (len < 32) throw Error(code, malformed + "too short");
  // the mask element, big-endian: two bits
  for (size_t i = 0; i < 31; i++)
    if (blob[i]) throw Error(code, malformed + "commitment mask out of range");
  if (blob[31] >> 2) throw Error(code, malformed + "commitment mask out of range");
  const size_t head = 32 + 64 * (2 - (size_t)__builtin_popcount(blob[31]));
  if (len < head + 32 || (len - head) % 32 != 0) throw Error(code, malformed + "wrong length");
  return (len - head) / 32;
}
// A blob read back; x.size() is its number of public inputs.  code: LH_ERR_ARG at a prover, whose call the blob is part of,
// LH_ERR_INVALID_SNARK at a verifier
NovaInstance read_instance(const char* name, int code, const uint8_t* blob, size_t len) {
  const std::string malformed = std::string(name) + ": malformed instance: ";
  const size_t p = instance_num_public(malformed, code, blob, len);
  KeccakTranscript kt;
  kt.stream.assign(blob, blob + len);
  Transcript tr(&kt.vt);
  NovaInstance U;
  try {
    const std::vector<HG1> comms = lasso_read_commitments(tr, 2);
    U.cw = comms[0], U.ce = comms[1];
    U.x = tr.read_field_elements(p);
  } catch (const Error& e) {
    throw Error(code, malformed + e.msg);
  }
  if (kt.pos != kt.stream.size()) throw Error(code, malformed + "wrong length");
  return U;
}
void absorb_instance(Transcript& tr, const NovaInstance& U) {
  argument_absorb_commitments(tr, {U.cw, U.ce});
  for (const HFr& v : U.x) tr.common_field_element(v);
}
HG1 g1_lincomb(const HG1& a, const HG1& b, const HFr& s) {  // a + s b
  return host::g1_to_affine(host::g1_add(host::g1_from_affine(a), host::g1_mul(host::g1_from_affine(b), s)));
}
// step 4's instance half: x1 + r x2, C_W1 + r C_W2, C_E1 + r C_T + r^2 C_E2
NovaInstance fold_instances(const NovaInstance& U1, const NovaInstance& U2, const HG1& ct, const HFr& r) {
  NovaInstance U;
  U.cw = g1_lincomb(U1.cw, U2.cw, r);
  U.ce = g1_lincomb(g1_lincomb(U1.ce, ct, r), U2.ce, r * r);
  U.x.resize(U1.x.size());
  for (size_t i = 0; i < U.x.size(); i++) U.x[i] = U1.x[i] + r * U2.x[i];
  return U;
}
// the caller's buffer takes any instance of p public inputs: checked before any work
void require_room(size_t room, size_t p) {
  LH_REQUIRE(room >= LH_NOVA_INSTANCE_BYTES(p), LH_ERR_ARG, "nova: the buffer is shorter than LH_NOVA_INSTANCE_BYTES(num_public)");
}
std::string unsatisfied_words(size_t bad, size_t l) {
  return "does not satisfy " + std::to_string(bad) + " of the 2^" + std::to_string(l) + " constraints";
}
Fr to_dev(const HFr& v) {
  Fr out;
  memcpy(&out, &v, sizeof(out));
  return out;
}
void spmv2(Ctx& c, const R1csKey& key, int direction, const Fr* X1, const Fr* X2, Fr* const* out1, Fr* const* out2) {
  NovaSpmv2 a;
  memset(&a, 0, sizeof(a));
  for (size_t m = 0; m < 3; m++) {
    a.seg[m] = key.seg[direction][m], a.other[m] = key.other[direction][m], a.perm[m] = key.perm[direction][m];
    a.val[m] = key.mat[m]->val, a.out1[m] = out1[m], a.out2[m] = out2[m];
  }
  a.X1 = X1, a.X2 = X2;
  k_nova_spmv2(c, a, (size_t)1 << key.n, key.l);
}
lh_sop relaxed_outer_expression(const HFr& u) {  // eq(tau, .) (Poly0 Poly1 - u Poly2 - Poly3)
  lh_sop sop;
  memset(&sop, 0, sizeof(sop));
  sop.num_terms = 3, sop.global_eq = 0;
  const HFr one = HFr::one(), minus_u = HFr::zero() - u, minus = HFr::zero() - HFr::one();
  memcpy(&sop.coeff[0], &one, 32), memcpy(&sop.coeff[1], &minus_u, 32), memcpy(&sop.coeff[2], &minus, 32);
  sop.num_factors[0] = 2, sop.factor[0][0] = 0, sop.factor[0][1] = 1;
  sop.num_factors[1] = 1, sop.factor[1][0] = 2;
  sop.num_factors[2] = 1, sop.factor[2][0] = 3;
  return sop;
}
// a verifier entry's verdict under `name`, as spartan_verify gives it
void verdict(const std::string& name, const std::function<void()>& verify) {
  try {
    argument_verdict(name, verify);
  } catch (const Error& e) {
    if (e.code != LH_ERR_INVALID_SNARK || e.msg.rfind(name + ": ", 0) == 0) throw;
    throw Error(LH_ERR_INVALID_SNARK, name + ": " + e.msg);
  }
}
}  // namespace

std::vector<uint8_t> nova_instance(Ctx& c, const Pcs& pcs, const R1csKey& key, const Fr* d_w, const HFr* x, size_t p, size_t room) {
  spartan_require_key(c, key, "nova");
  const size_t n = key.n, l = key.l;
  const size_t nv = spartan_check(n, l, p);
  require_room(room, p);
  LH_REQUIRE(d_w != nullptr && x != nullptr, LH_ERR_ARG, "null argument: d_w or x");
  argument_not_sharded(c, "nova");
  argument_pcs_check(pcs, nv, "nova", true);
  LH_REQUIRE(x[0] == HFr::one(), LH_ERR_ARG, "nova: a fresh instance has x[0] = 1 (the relaxation scalar u is x[0])");
  const size_t M = (size_t)1 << l;
  open_precommit_cancel(c);
  ArenaScope scope(c.arena);
  Fr* z = c.arena.alloc_n<Fr>(M);
  spartan_assignment(c, l, d_w, x, p, z);
  Fr* Mz[3];
  for (Fr*& t : Mz) t = c.arena.alloc_n<Fr>(M);
  spartan_spmv(c, key, 0, z, Mz);
  const size_t bad = k_spartan_unsatisfied(c, Mz[0], Mz[1], Mz[2], M);
  LH_REQUIRE(bad == 0, LH_ERR_ARG, "nova: the witness " + unsatisfied_words(bad, l));
  NovaInstance U;
  U.cw = pcs.batch_commit(&d_w, 1, l - 1)[0];
  U.ce = HG1{host::Fq::zero(), host::Fq::zero()};
  U.x.assign(x, x + p);
  return instance_blob(U);
}

std::vector<uint8_t> nova_fold(Ctx& c, const Pcs& pcs, const R1csKey& key, const uint8_t* blob1, size_t len1, const uint8_t* blob2,
                               size_t len2, const Fr* d_w1, const Fr* d_e1, const Fr* d_w2, const Fr* d_e2, Fr* d_w_out, Fr* d_e_out,
                               size_t room, Transcript& tr) {
  spartan_require_key(c, key, "nova");
  const size_t n = key.n, l = key.l;
  LH_REQUIRE(blob1 && blob2 && d_w1 && d_w2 && d_w_out && d_e_out, LH_ERR_ARG, "null argument: a blob, a witness or an output");
  const NovaInstance U1 = read_instance("nova", LH_ERR_ARG, blob1, len1), U2 = read_instance("nova", LH_ERR_ARG, blob2, len2);
  const size_t p = U1.x.size();
  LH_REQUIRE(U2.x.size() == p, LH_ERR_ARG, "nova: the two instances have different numbers of public inputs");
  const size_t nv = spartan_check(n, l, p);
  require_room(room, p);
  argument_not_sharded(c, "nova");
  argument_pcs_check(pcs, nv, "nova", true);
  const size_t M = (size_t)1 << l, half = M / 2;
  open_precommit_cancel(c);
  ArenaScope scope(c.arena);
  // ---- 0: z1, z2, the six products in one pass over the sorted streams, T and the rows that fail - no challenge is needed:
  // an input that does not satisfy its relation is refused before the transcript is touched
  Fr *z1 = c.arena.alloc_n<Fr>(M), *z2 = c.arena.alloc_n<Fr>(M);
  spartan_assignment(c, l, d_w1, U1.x.data(), p, z1);
  spartan_assignment(c, l, d_w2, U2.x.data(), p, z2);
  Fr *Mz1[3], *Mz2[3];
  for (Fr*& t : Mz1) t = c.arena.alloc_n<Fr>(M);
  for (Fr*& t : Mz2) t = c.arena.alloc_n<Fr>(M);
  spmv2(c, key, 0, z1, z2, Mz1, Mz2);
  Fr* T = c.arena.alloc_n<Fr>(M);
  NovaCross x;
  for (size_t m = 0; m < 3; m++) x.mz1[m] = Mz1[m], x.mz2[m] = Mz2[m];
  x.e1 = d_e1, x.e2 = d_e2, x.t = T;
  size_t bad[2];
  k_nova_cross_term(c, x, to_dev(U1.x[0]), to_dev(U2.x[0]), M, bad);
  for (size_t k = 0; k < 2; k++)
    LH_REQUIRE(bad[k] == 0, LH_ERR_ARG, "nova: input " + std::to_string(k + 1) + " " + unsatisfied_words(bad[k], l));
  // ---- 1/2/3: the statement; the commitment of T; r
  std::vector<HG1> comms[3];
  for (size_t m = 0; m < 3; m++) comms[m] = key.mat[m]->comms;
  spartan_key_header(tr, n, l, p, comms);
  absorb_instance(tr, U1);
  absorb_instance(tr, U2);
  const Fr* t_poly = T;
  const std::vector<HG1> ct = pcs.batch_commit(&t_poly, 1, l);
  lasso_write_commitments(tr, ct);
  const HFr r = tr.squeeze_challenge();
  // ---- 4: the witness on the device, the instance on the host
  k_nova_fold(c, d_w1, d_w2, d_w_out, d_e1, T, d_e2, d_e_out, to_dev(r), to_dev(r * r), half, M);
  const std::vector<uint8_t> out = instance_blob(fold_instances(U1, U2, ct[0], r));
  c.sync();
  return out;
}

std::vector<uint8_t> nova_fold_verify(size_t n, size_t l, const uint8_t* key, size_t key_len, const uint8_t* blob1, size_t len1,
                                      const uint8_t* blob2, size_t len2, size_t room, Transcript& tr) {
  spartan_check(n, l, 1);
  LH_REQUIRE(key && blob1 && blob2, LH_ERR_ARG, "null argument: key or a blob");
  std::vector<uint8_t> out;
  verdict("nova", [&] {
    const NovaInstance U1 = read_instance("nova", LH_ERR_INVALID_SNARK, blob1, len1);
    const NovaInstance U2 = read_instance("nova", LH_ERR_INVALID_SNARK, blob2, len2);
    const size_t p = U1.x.size();
    if (U2.x.size() != p) throw Error(LH_ERR_INVALID_SNARK, "nova: the two instances have different numbers of public inputs");
    if (p > (size_t)1 << (l - 1)) throw Error(LH_ERR_INVALID_SNARK, "nova: malformed instance: more public inputs than 2^(dim_vars - 1)");
    require_room(room, p);  // (blobs that can be read say how much room their fold takes: LH_ERR_ARG, before a byte is read)
    const SpartanKeyBlob k = spartan_read_key("nova", key, key_len);
    spartan_key_header(tr, n, l, p, k.comms);
    absorb_instance(tr, U1);
    absorb_instance(tr, U2);
    const HG1 ct = lasso_read_commitments(tr, 1)[0];
    const HFr r = tr.squeeze_challenge();
    out = instance_blob(fold_instances(U1, U2, ct, r));
  });
  return out;
}

void spartan_prove_relaxed(Ctx& c, const Pcs& pcs, const R1csKey& key, const uint8_t* blob, size_t len, const Fr* d_w, const Fr* d_e,
                           Transcript& tr) {
  spartan_require_key(c, key, "spartan");
  const size_t n = key.n, l = key.l;
  LH_REQUIRE(blob != nullptr && d_w != nullptr, LH_ERR_ARG, "null argument: the instance or d_w");
  const NovaInstance U = read_instance("spartan", LH_ERR_ARG, blob, len);
  const size_t p = U.x.size();
  const size_t nv = spartan_check(n, l, p);
  argument_not_sharded(c, "spartan");
  argument_pcs_check(pcs, nv, "spartan", true);
  LH_REQUIRE(d_e != nullptr || U.ce.is_identity(), LH_ERR_ARG, "null argument: d_e (the instance's C_E is not the identity)");
  const HFr u = U.x[0];
  const size_t M = (size_t)1 << l;
  open_precommit_cancel(c);
  std::vector<HFr> r_x, r_y, e;
  {
    ArenaScope scope(c.arena);
    EqHalfScope eq_scope(c);
    // ---- an E beside a C_E that is the identity has to be zero (E E != 0 counts its non-zero rows: the field has no zero
    // divisors); z, Az, Bz, Cz and the rows that fail the relaxed relation.  All refused before the transcript is touched
    if (d_e && U.ce.is_identity())
      LH_REQUIRE(k_nova_unsatisfied(c, d_e, d_e, d_e, to_dev(HFr::zero()), nullptr, M) == 0, LH_ERR_ARG,
                 "spartan: the instance's C_E is the identity but E is not zero");
    Fr* z = c.arena.alloc_n<Fr>(M);
    spartan_assignment(c, l, d_w, U.x.data(), p, z);
    Fr* Mz[3];
    for (Fr*& t : Mz) t = c.arena.alloc_n<Fr>(M);
    spartan_spmv(c, key, 0, z, Mz);
    const size_t bad = k_nova_unsatisfied(c, Mz[0], Mz[1], Mz[2], to_dev(u), d_e, M);
    LH_REQUIRE(bad == 0, LH_ERR_ARG, "spartan: the witness " + unsatisfied_words(bad, l));
    const Fr* E = d_e;
    if (!E) {  // (a fresh instance: the fourth table of the outer sum-check is zero)
      Fr* zero = c.arena.alloc_n<Fr>(M);
      LH_HIP(hipMemsetAsync(zero, 0, M * sizeof(Fr), c.stream));
      E = zero;
    }
    // ---- the header: the key, then the instance (C_W is part of it: nothing is written); tau
    std::vector<HG1> comms[3];
    for (size_t m = 0; m < 3; m++) comms[m] = key.mat[m]->comms;
    spartan_key_header(tr, n, l, p, comms);
    absorb_instance(tr, U);
    const std::vector<HFr> tau = tr.squeeze_challenges(l);
    // ---- the outer sum-check, claim 0 (exact: the count above), then Az, Bz, Cz, E at r_x
    ScOptions so;
    so.sum_is_exact = true;
    std::vector<HFr> at_rx;
    {
      const Fr* polys[4] = {Mz[0], Mz[1], Mz[2], E};
      SumCheckResult sc = sum_check_prove(c, LH_SC_EVALUATIONS, l, relaxed_outer_expression(u), polys, 4, tau.data(), 1, HFr::zero(), tr, so);
      r_x = sc.challenges, at_rx = sc.evals;
    }
    tr.write_field_elements(at_rx);
    // ---- the inner half, as the plain prover's; then E at r_x over l variables
    spartan_inner_prove(c, pcs, key, z, d_w, Mz, r_x, at_rx.data(), tr, r_y, e);
    if (!U.ce.is_identity()) {
      const std::vector<lh_evaluation> evs = spartan_doubled_evaluation(at_rx[3]);
      pcs.batch_open(l, &E, 1, r_x.data(), 1, evs.data(), evs.size(), tr, nullptr);
    }
  }
  spartan_open_matrices(c, pcs, key, r_x, r_y, e, tr);
}

void spartan_verify_relaxed(const PcsVerifier& pcs, size_t n, size_t l, const uint8_t* key, size_t key_len, const uint8_t* blob,
                            size_t len, size_t p, Transcript& tr) {
  spartan_check(n, l, p);
  LH_REQUIRE(key != nullptr && blob != nullptr, LH_ERR_ARG, "null argument: key or the instance");
  argument_pcs_check(pcs, "spartan");
  verdict("spartan", [&] {
    const SpartanKeyBlob k = spartan_read_key("spartan", key, key_len);
    const NovaInstance U = read_instance("spartan", LH_ERR_INVALID_SNARK, blob, len);
    if (U.x.size() != p) throw Error(LH_ERR_INVALID_SNARK, "spartan: malformed instance: not of num_public public inputs");
    const HFr u = U.x[0];
    spartan_key_header(tr, n, l, p, k.comms);
    absorb_instance(tr, U);
    const std::vector<HFr> tau = tr.squeeze_challenges(l);
    const std::pair<HFr, std::vector<HFr>> outer = sum_check_verify(LH_SC_EVALUATIONS, l, 3, HFr::zero(), tr);
    const std::vector<HFr>& r_x = outer.second;
    const std::vector<HFr> v = tr.read_field_elements(4);
    if (U.ce.is_identity() && !v[3].is_zero()) throw Error(LH_ERR_INVALID_SNARK, "spartan: vE is not zero though C_E is the identity");
    if (outer.first != host_eq_xy_eval(tau.data(), r_x.data(), l) * (v[0] * v[1] - u * v[2] - v[3]))
      throw Error(LH_ERR_INVALID_SNARK, "spartan: outer sum-check final evaluation mismatch");
    std::vector<HFr> r_y, e;
    spartan_inner_verify(pcs, l, U.x.data(), p, U.cw, v.data(), tr, r_y, e);
    if (!U.ce.is_identity()) {
      const std::vector<lh_evaluation> evs = spartan_doubled_evaluation(v[3]);
      pcs.batch_verify(l, &U.ce, 1, r_x.data(), 1, evs.data(), evs.size(), tr);
    }
    spartan_verify_matrices(pcs, n, l, k, r_x, r_y, e, tr);
  });
}

void nova_debug_spmv2(Ctx& c, const R1csKey& key, int direction, const Fr* d_x1, const Fr* d_x2, Fr* const* d_out1, Fr* const* d_out2) {
  spartan_require_key(c, key, "nova");
  LH_REQUIRE(direction == 0 || direction == 1, LH_ERR_ARG, "nova: direction is 0 (by rows) or 1 (by columns)");
  LH_REQUIRE(d_x1 && d_x2 && d_out1 && d_out2, LH_ERR_ARG, "null argument: d_x or d_out");
  for (size_t m = 0; m < 3; m++) LH_REQUIRE(d_out1[m] && d_out2[m], LH_ERR_ARG, "null argument: d_x or d_out");
  spmv2(c, key, direction, d_x1, d_x2, d_out1, d_out2);
  c.sync();
}

}  // namespace lh
