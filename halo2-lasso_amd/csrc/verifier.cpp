// The verify half of the trait surface, host only (no GPU work: a verifier reads a few KB of proof and does
// O(num_vars) field operations and pairings).
//   SumCheck::verify                       piop/sum_check/classic.rs:175-193,242-272, eval.rs:34-57, coeff.rs:19-39
//   MultilinearKzg::{verify, batch_verify} pcs/multilinear/kzg.rs:330-375, pcs/multilinear.rs:237-276
//   HyperPlonk::verify                     backend/hyperplonk.rs:293-362, hyperplonk/verifier.rs:39-182,
//                                          piop/sum_check.rs:60-125, poly/multilinear.rs:433-475
//   Lasso verify                           oracle/pyref/lasso.py (the build's own protocol; no reference code)
//   MultilinearBrakedown::verify           pcs/multilinear/brakedown.rs:315-396 (two rows re-encoded on the host)
//   UnivariateKzg / Gemini verify          pcs/univariate/kzg.rs:366-555, pcs/multilinear/gemini.rs:165-211
#include <algorithm>
#include <map>
#include <set>
#include <string>
#include "host.hpp"
#include "expr.hpp"
#include "pairing.hpp"
#include "brakedown.hpp"

namespace lh {

using host::G2Affine;

struct VerifierParams {
  HG1 g1;
  G2Affine g2;
  std::vector<G2Affine> ss;
};

static G2Affine g2_from_c(const lh_g2& p) {
  G2Affine a;
  static_assert(sizeof(lh_g2) == sizeof(G2Affine), "lh_g2 layout");
  memcpy(&a, &p, sizeof(a));
  return a;
}
static lh_g2 g2_to_c(const G2Affine& a) {
  lh_g2 p;
  memcpy(&p, &a, sizeof(p));
  return p;
}

VerifierParams* mkzg_vp_setup(const HFr* ss, size_t num_vars) {
  auto* vp = new VerifierParams();
  vp->g1 = HG1{host::Fq::from_u64(1), host::Fq::from_u64(2)};
  vp->g2 = host::g2_generator();
  host::G2Xyzz g = host::g2_from_affine(vp->g2);
  for (size_t i = 0; i < num_vars; i++) vp->ss.push_back(host::g2_to_affine(host::g2_mul(g, ss[i])));
  return vp;
}
VerifierParams* mkzg_vp_new(const lh_g1& g1, const lh_g2& g2, const lh_g2* ss, size_t num_vars) {
  auto* vp = new VerifierParams();
  memcpy(&vp->g1, &g1, sizeof(HG1));
  vp->g2 = g2_from_c(g2);
  bool ok = host::g2_is_on_curve(vp->g2);
  for (size_t i = 0; i < num_vars; i++) {
    vp->ss.push_back(g2_from_c(ss[i]));
    ok = ok && host::g2_is_on_curve(vp->ss.back());
  }
  if (!ok) {
    delete vp;
    throw Error(LH_ERR_SERIALIZATION, "verifier params: G2 point not on the curve");
  }
  return vp;
}
void mkzg_vp_export(const VerifierParams& vp, lh_g1* g1, lh_g2* g2, lh_g2* ss) {
  if (g1) memcpy(g1, &vp.g1, sizeof(HG1));
  if (g2) *g2 = g2_to_c(vp.g2);
  if (ss)
    for (size_t i = 0; i < vp.ss.size(); i++) ss[i] = g2_to_c(vp.ss[i]);
}
size_t mkzg_vp_num_vars(const VerifierParams& vp) { return vp.ss.size(); }
void mkzg_vp_free(VerifierParams* vp) { delete vp; }

bool pairing_check(const lh_g1* ps, const lh_g2* qs, size_t n) {
  std::vector<std::pair<HG1, G2Affine>> pairs(n);
  for (size_t i = 0; i < n; i++) {
    memcpy(&pairs[i].first, &ps[i], sizeof(HG1));
    pairs[i].second = g2_from_c(qs[i]);
    LH_REQUIRE(host::g2_is_on_curve(pairs[i].second), LH_ERR_ARG, "pairing: G2 point not on the curve");
  }
  return host::pairings_product_is_identity(pairs);
}

// ------------------------------------------------------------------ SumCheck::verify
std::pair<HFr, std::vector<HFr>> sum_check_verify(int prover_kind, size_t num_vars, size_t degree, const HFr& sum,
                                                  Transcript& tr) {
  LH_REQUIRE(prover_kind == LH_SC_EVALUATIONS || prover_kind == LH_SC_COEFFICIENTS, LH_ERR_ARG, "bad prover kind");
  std::vector<std::vector<HFr>> msgs;
  std::vector<HFr> challenges;
  for (size_t r = 0; r < num_vars; r++) {  // classic.rs:250-258: all messages first, then the consistency pass
    msgs.push_back(tr.read_field_elements(degree + 1));
    challenges.push_back(tr.squeeze_challenge());
  }
  HFr s = sum;
  for (size_t r = 0; r < num_vars; r++) {
    const std::vector<HFr>& m = msgs[r];
    HFr msg_sum;
    if (prover_kind == LH_SC_EVALUATIONS) {
      msg_sum = m[0] + (m.size() > 1 ? m[1] : HFr::zero());
    } else {
      msg_sum = m[0].dbl();
      for (size_t i = 1; i < m.size(); i++) msg_sum += m[i];
    }
    if (s != msg_sum)
      throw Error(LH_ERR_INVALID_SUMCHECK,
                  r == 0 ? std::string("Expect sum to match the first round message")
                         : "Consistency failure at round " + std::to_string(r));
    s = prover_kind == LH_SC_EVALUATIONS ? interpolate_evals(m, challenges[r]) : horner(m, challenges[r]);
  }
  return {s, challenges};
}

// ------------------------------------------------------------------ MultilinearKzg::verify / batch_verify
void mkzg_verify(const VerifierParams& vp, const HG1& comm, const HFr* point, size_t num_vars, const HFr& eval,
                 Transcript& tr) {
  if (num_vars > vp.ss.size())
    throw Error(LH_ERR_INVALID_PCS_PARAM, "Too many variates of poly to verify (param supports variates up to " +
                                              std::to_string(vp.ss.size()) + " but got " + std::to_string(num_vars) + ")");
  std::vector<HG1> quotients = tr.read_commitments(num_vars);
  std::vector<std::pair<HG1, G2Affine>> pairs;
  host::G1Xyzz lhs0 = host::g1_add(host::g1_from_affine(comm),
                                   host::g1_mul(host::g1_from_affine(HG1{vp.g1.x, -vp.g1.y}), eval));
  pairs.push_back({host::g1_to_affine(lhs0), host::g2_neg(vp.g2)});
  host::G2Xyzz g2 = host::g2_from_affine(vp.g2);
  for (size_t i = 0; i < num_vars; i++) {
    host::G2Xyzz rhs = host::g2_add(host::g2_from_affine(vp.ss[i]), host::g2_mul(g2, -point[i]));
    pairs.push_back({quotients[i], host::g2_to_affine(rhs)});
  }
  if (!host::pairings_product_is_identity(pairs)) throw Error(LH_ERR_INVALID_PCS_OPEN, "Invalid multilinear KZG open");
}

// additive::batch_verify (pcs/multilinear.rs:237-276), generic over the PCS
// the part every commitment type shares: -> (scalar of every evaluation's commitment, challenges x, g'(x))
struct AdditiveClaim {
  std::vector<HFr> scalars, x;
  HFr eval;
};
static AdditiveClaim additive_batch_claim(size_t num_vars, size_t num_comms, const HFr* points, size_t num_points,
                                          const lh_evaluation* evals, size_t num_evals, Transcript& tr) {
  for (size_t i = 0; i < num_evals; i++)
    LH_REQUIRE(evals[i].poly < num_comms && evals[i].point < num_points, LH_ERR_ARG, "batch verify: bad evaluation");
  size_t ell = 0;
  while (((size_t)1 << ell) < num_evals) ell++;
  std::vector<HFr> t = tr.squeeze_challenges(ell);
  std::vector<HFr> eq_xt = host_eq_xy(t);
  HFr tilde_gs_sum = HFr::zero();
  for (size_t i = 0; i < num_evals; i++) {
    HFr v;
    memcpy(&v, &evals[i].value, 32);
    tilde_gs_sum += v * eq_xt[i];
  }
  auto res = sum_check_verify(LH_SC_COEFFICIENTS, num_vars, 2, tilde_gs_sum, tr);
  const std::vector<HFr>& x = res.second;
  std::vector<HFr> eq_evals(num_points);
  for (size_t j = 0; j < num_points; j++) eq_evals[j] = host_eq_xy_eval(x.data(), points + j * num_vars, num_vars);
  AdditiveClaim out;
  out.x = x, out.eval = res.first;
  for (size_t i = 0; i < num_evals; i++) out.scalars.push_back(eq_evals[evals[i].point] * eq_xt[i]);
  return out;
}
static void additive_batch_verify(size_t num_vars, const HG1* comms, size_t num_comms, const HFr* points,
                                  size_t num_points, const lh_evaluation* evals, size_t num_evals, Transcript& tr,
                                  const std::function<void(const HG1&, const HFr*, const HFr&)>& verify) {
  const AdditiveClaim cl = additive_batch_claim(num_vars, num_comms, points, num_points, evals, num_evals, tr);
  host::G1Xyzz acc = host::G1Xyzz::identity();  // sum_with_scalar (kzg.rs:138-149)
  for (size_t i = 0; i < num_evals; i++)
    acc = host::g1_add(acc, host::g1_mul(host::g1_from_affine(comms[evals[i].poly]), cl.scalars[i]));
  verify(host::g1_to_affine(acc), cl.x.data(), cl.eval);
}
// the same over commitments that are vectors of `chunks` points (Hyrax's sum_with_scalar, hyrax.rs:80-107: chunk by chunk)
static void additive_batch_verify_chunks(size_t num_vars, const HG1* comms, size_t num_comms, size_t chunks, const HFr* points,
                                         size_t num_points, const lh_evaluation* evals, size_t num_evals, Transcript& tr,
                                         const std::function<void(const HG1*, const HFr*, const HFr&)>& verify) {
  const AdditiveClaim cl = additive_batch_claim(num_vars, num_comms, points, num_points, evals, num_evals, tr);
  std::vector<host::G1Xyzz> acc(chunks, host::G1Xyzz::identity());
  host_parallel_for(chunks, [&](size_t k) {
    for (size_t i = 0; i < num_evals; i++)
      acc[k] = host::g1_add(acc[k], host::g1_mul(host::g1_from_affine(comms[(size_t)evals[i].poly * chunks + k]), cl.scalars[i]));
  });
  std::vector<HG1> sum(chunks);
  host::g1_batch_to_affine(acc.data(), chunks, sum.data());
  verify(sum.data(), cl.x.data(), cl.eval);
}

void mkzg_batch_verify(const VerifierParams& vp, size_t num_vars, const HG1* comms, size_t num_comms,
                       const HFr* points, size_t num_points, const lh_evaluation* evals, size_t num_evals,
                       Transcript& tr) {
  if (num_vars > vp.ss.size())
    throw Error(LH_ERR_INVALID_PCS_PARAM,
                "Too many variates of poly to batch verify (param supports variates up to " +
                    std::to_string(vp.ss.size()) + " but got " + std::to_string(num_vars) + ")");
  additive_batch_verify(num_vars, comms, num_comms, points, num_points, evals, num_evals, tr,
                        [&](const HG1& comm, const HFr* x, const HFr& eval) { mkzg_verify(vp, comm, x, num_vars, eval, tr); });
}
// the scheme as a verifier's PCS: its batch_verify with the param bound (`args`: the arguments of PcsBatchVerify)
PcsVerifier mkzg_verifier(const VerifierParams& vp) {
  return {[&vp](auto&&... args) { mkzg_batch_verify(vp, args...); }};
}

// ------------------------------------------------------------------ Zeromorph::verify (zeromorph.rs:215-256)
struct ZmVerifierParams {
  HG1 g1;
  G2Affine g2, s_g2, s_offset_g2;
};
ZmVerifierParams* zeromorph_vp_setup(const HFr& s, size_t param_size, size_t poly_size) {
  LH_REQUIRE(poly_size >= 1 && poly_size <= param_size, LH_ERR_INVALID_PCS_PARAM, "Too large poly_size to trim to");
  auto* vp = new ZmVerifierParams();
  vp->g1 = HG1{host::Fq::from_u64(1), host::Fq::from_u64(2)};
  vp->g2 = host::g2_generator();
  host::G2Xyzz g = host::g2_from_affine(vp->g2);
  vp->s_g2 = host::g2_to_affine(host::g2_mul(g, s));
  HFr so = HFr::one();  // s^(param_size - poly_size)
  for (size_t i = 0; i < param_size - poly_size; i++) so *= s;
  vp->s_offset_g2 = host::g2_to_affine(host::g2_mul(g, so));
  return vp;
}
ZmVerifierParams* zeromorph_vp_new(const lh_g1& g1, const lh_g2& g2, const lh_g2& s_g2, const lh_g2& s_offset_g2) {
  auto* vp = new ZmVerifierParams();
  memcpy(&vp->g1, &g1, sizeof(HG1));
  vp->g2 = g2_from_c(g2), vp->s_g2 = g2_from_c(s_g2), vp->s_offset_g2 = g2_from_c(s_offset_g2);
  if (!host::g2_is_on_curve(vp->g2) || !host::g2_is_on_curve(vp->s_g2) || !host::g2_is_on_curve(vp->s_offset_g2)) {
    delete vp;
    throw Error(LH_ERR_SERIALIZATION, "verifier params: G2 point not on the curve");
  }
  return vp;
}
void zeromorph_vp_export(const ZmVerifierParams& vp, lh_g1* g1, lh_g2* g2, lh_g2* s_g2, lh_g2* s_offset_g2) {
  if (g1) memcpy(g1, &vp.g1, sizeof(HG1));
  if (g2) *g2 = g2_to_c(vp.g2);
  if (s_g2) *s_g2 = g2_to_c(vp.s_g2);
  if (s_offset_g2) *s_offset_g2 = g2_to_c(vp.s_offset_g2);
}
void zeromorph_vp_free(ZmVerifierParams* vp) { delete vp; }

void zeromorph_verify(const ZmVerifierParams& vp, const HG1& comm, const HFr* point, size_t num_vars, const HFr& eval,
                      Transcript& tr) {
  std::vector<HG1> q_comms = tr.read_commitments(num_vars);
  const HFr y = tr.squeeze_challenge();
  const HG1 q_hat_comm = tr.read_commitment();
  const HFr x = tr.squeeze_challenge(), z = tr.squeeze_challenge();
  auto sc = zeromorph_scalars(y, x, z, point, num_vars);
  host::G1Xyzz c = host::g1_from_affine(q_hat_comm);
  c = host::g1_add(c, host::g1_mul(host::g1_from_affine(comm), z));
  c = host::g1_add(c, host::g1_mul(host::g1_from_affine(vp.g1), sc.first * eval));
  for (size_t k = 0; k < num_vars; k++) c = host::g1_add(c, host::g1_mul(host::g1_from_affine(q_comms[k]), sc.second[k]));
  const HG1 pi = tr.read_commitment();
  host::G2Xyzz rhs = host::g2_add(host::g2_from_affine(vp.s_g2), host::g2_mul(host::g2_from_affine(vp.g2), -x));
  if (!host::pairings_product_is_identity({{host::g1_to_affine(c), host::g2_neg(vp.s_offset_g2)},
                                            {pi, host::g2_to_affine(rhs)}}))
    throw Error(LH_ERR_INVALID_PCS_OPEN, "Invalid Zeromorph KZG open");
}
void zeromorph_batch_verify(const ZmVerifierParams& vp, size_t num_vars, const HG1* comms, size_t num_comms,
                            const HFr* points, size_t num_points, const lh_evaluation* evals, size_t num_evals,
                            Transcript& tr) {
  additive_batch_verify(num_vars, comms, num_comms, points, num_points, evals, num_evals, tr,
                        [&](const HG1& comm, const HFr* x, const HFr& eval) { zeromorph_verify(vp, comm, x, num_vars, eval, tr); });
}
PcsVerifier zeromorph_verifier(const ZmVerifierParams& vp) {
  return {[&vp](auto&&... args) { zeromorph_batch_verify(vp, args...); }};
}

// ------------------------------------------------------------------ UnivariateKzg::{verify, batch_verify} (univariate/kzg.rs:366-555)
struct UkzgVerifierParams {
  HG1 g1;
  G2Affine g2, s_g2;
};
UkzgVerifierParams* ukzg_vp_setup(const HFr& s) {
  auto* vp = new UkzgVerifierParams();
  vp->g1 = HG1{host::Fq::from_u64(1), host::Fq::from_u64(2)};
  vp->g2 = host::g2_generator();
  vp->s_g2 = host::g2_to_affine(host::g2_mul(host::g2_from_affine(vp->g2), s));
  return vp;
}
UkzgVerifierParams* ukzg_vp_new(const lh_g1& g1, const lh_g2& g2, const lh_g2& s_g2) {
  auto* vp = new UkzgVerifierParams();
  memcpy(&vp->g1, &g1, sizeof(HG1));
  vp->g2 = g2_from_c(g2), vp->s_g2 = g2_from_c(s_g2);
  if (!host::g2_is_on_curve(vp->g2) || !host::g2_is_on_curve(vp->s_g2)) {
    delete vp;
    throw Error(LH_ERR_SERIALIZATION, "verifier params: G2 point not on the curve");
  }
  return vp;
}
void ukzg_vp_export(const UkzgVerifierParams& vp, lh_g1* g1, lh_g2* g2, lh_g2* s_g2) {
  if (g1) memcpy(g1, &vp.g1, sizeof(HG1));
  if (g2) *g2 = g2_to_c(vp.g2);
  if (s_g2) *s_g2 = g2_to_c(vp.s_g2);
}
void ukzg_vp_free(UkzgVerifierParams* vp) { delete vp; }

// kzg.rs:366-378: c = pi * point + comm - g1 * eval;  e(c, -g2) e(pi, [s]_2) == 1
void ukzg_verify(const UkzgVerifierParams& vp, const HG1& comm, const HFr& point, const HFr& eval, Transcript& tr) {
  const HG1 pi = tr.read_commitment();
  host::G1Xyzz c = host::g1_mul(host::g1_from_affine(pi), point);
  c = host::g1_add(c, host::g1_from_affine(comm));
  c = host::g1_add(c, host::g1_mul(host::g1_from_affine(HG1{vp.g1.x, -vp.g1.y}), eval));
  if (!host::pairings_product_is_identity({{host::g1_to_affine(c), host::g2_neg(vp.g2)}, {pi, vp.s_g2}}))
    throw Error(LH_ERR_INVALID_PCS_OPEN, "Invalid univariate KZG open");
}

// kzg.rs:454-512: polys grouped by their point set (as a set), in order of first appearance
UkzgEvalSets ukzg_eval_sets(const lh_evaluation* evals, size_t num_evals) {
  struct Shift {
    size_t poly;
    std::vector<size_t> points;
    std::vector<HFr> values;
  };
  std::vector<Shift> shifts;
  std::set<size_t> superset;
  for (size_t i = 0; i < num_evals; i++) {
    const size_t poly = evals[i].poly, point = evals[i].point;
    HFr v;
    memcpy(&v, &evals[i].value, 32);
    size_t pos = 0;
    while (pos < shifts.size() && shifts[pos].poly != poly) pos++;
    if (pos == shifts.size()) {
      shifts.push_back(Shift{poly, {point}, {v}});
    } else if (std::find(shifts[pos].points.begin(), shifts[pos].points.end(), point) == shifts[pos].points.end()) {
      shifts[pos].points.push_back(point);
      shifts[pos].values.push_back(v);
    }
    superset.insert(point);
  }
  UkzgEvalSets out;
  out.superset.assign(superset.begin(), superset.end());
  for (const Shift& sh : shifts) {
    const std::set<size_t> key(sh.points.begin(), sh.points.end());
    size_t pos = 0;
    while (pos < out.sets.size() && std::set<size_t>(out.sets[pos].points.begin(), out.sets[pos].points.end()) != key) pos++;
    if (pos == out.sets.size()) {
      UkzgEvalSet st;
      st.polys = {sh.poly}, st.points = sh.points, st.evals = {sh.values};
      for (size_t idx : out.superset)
        if (!key.count(idx)) st.diffs.push_back(idx);
      out.sets.push_back(std::move(st));
    } else {
      UkzgEvalSet& st = out.sets[pos];
      if (std::find(st.polys.begin(), st.polys.end(), sh.poly) != st.polys.end()) continue;
      st.polys.push_back(sh.poly);
      std::vector<HFr> ev;
      for (size_t lhs : st.points) ev.push_back(sh.values[std::find(sh.points.begin(), sh.points.end(), lhs) - sh.points.begin()]);
      st.evals.push_back(std::move(ev));
    }
  }
  return out;
}
HFr ukzg_vanishing_eval(const std::vector<size_t>& idx, const HFr* points, const HFr& z) {
  HFr acc = HFr::one();
  for (size_t i : idx) acc *= z - points[i];
  return acc;
}
// kzg.rs:514-533: normalised by the first set's scalar (fflonk), one when that is zero
std::pair<std::vector<HFr>, HFr> ukzg_set_scalars(const std::vector<UkzgEvalSet>& sets, const std::vector<HFr>& powers_of_gamma,
                                                  const HFr* points, const HFr& z) {
  std::vector<HFr> vde(sets.size());
  for (size_t s = 0; s < sets.size(); s++) vde[s] = ukzg_vanishing_eval(sets[s].diffs, points, z);
  const HFr normalizer = vde[0].is_zero() ? HFr::one() : vde[0].inv();
  std::vector<HFr> out(sets.size());
  for (size_t s = 0; s < sets.size(); s++) out[s] = normalizer * vde[s] * powers_of_gamma[s];
  return {out, normalizer};
}
// arithmetic.rs:108-136
static std::vector<HFr> barycentric_weights(const std::vector<HFr>& points) {
  std::vector<HFr> w(points.size());
  for (size_t j = 0; j < points.size(); j++) {
    HFr acc = HFr::one();
    for (size_t i = 0; i < points.size(); i++)
      if (i != j) acc *= points[j] - points[i];
    w[j] = acc.inv();
  }
  return w;
}
static HFr barycentric_interpolate(const std::vector<HFr>& weights, const std::vector<HFr>& points, const std::vector<HFr>& evals,
                                   const HFr& x) {
  HFr sum = HFr::zero(), acc = HFr::zero();
  for (size_t i = 0; i < points.size(); i++) {
    const HFr coeff = (x - points[i]).inv() * weights[i];
    sum += coeff;
    acc += coeff * evals[i];
  }
  LH_REQUIRE(!sum.is_zero(), LH_ERR_INVALID_PCS_OPEN, "Invalid univariate KZG open");  // (the reference unwraps the inverse)
  return acc * sum.inv();
}

void ukzg_batch_verify(const UkzgVerifierParams& vp, const HG1* comms, size_t num_comms, const HFr* points, size_t num_points,
                       const lh_evaluation* evals, size_t num_evals, Transcript& tr) {
  LH_REQUIRE(num_evals >= 1, LH_ERR_ARG, "univariate batch verify: no evaluations");
  for (size_t i = 0; i < num_evals; i++)
    LH_REQUIRE(evals[i].poly < num_comms && evals[i].point < num_points, LH_ERR_ARG, "univariate batch verify: bad evaluation");
  const UkzgEvalSets es = ukzg_eval_sets(evals, num_evals);
  const std::vector<UkzgEvalSet>& sets = es.sets;
  const HFr beta = tr.squeeze_challenge(), gamma = tr.squeeze_challenge();
  const HG1 q_comm = tr.read_commitment();
  const HFr z = tr.squeeze_challenge();
  size_t max_set_len = 0;
  for (auto& s : sets) max_set_len = std::max(max_set_len, s.polys.size());
  std::vector<HFr> pob(max_set_len), pog(sets.size());
  pob[0] = HFr::one();
  for (size_t i = 1; i < max_set_len; i++) pob[i] = pob[i - 1] * beta;
  pog[0] = HFr::one();
  for (size_t i = 1; i < sets.size(); i++) pog[i] = pog[i - 1] * gamma;
  auto sc = ukzg_set_scalars(sets, pog, points, z);
  std::vector<HFr> scalars(num_comms, HFr::zero());  // comm_scalars (kzg.rs:541-555)
  for (size_t s = 0; s < sets.size(); s++)
    for (size_t k = 0; k < sets[s].polys.size(); k++) scalars[sets[s].polys[k]] = sc.first[s] * pob[k];
  const HFr q_scalar = -(ukzg_vanishing_eval(es.superset, points, z) * sc.second);
  host::G1Xyzz f = host::g1_mul(host::g1_from_affine(q_comm), q_scalar);
  for (size_t i = 0; i < num_comms; i++)
    if (!scalars[i].is_zero()) f = host::g1_add(f, host::g1_mul(host::g1_from_affine(comms[i]), scalars[i]));
  HFr eval = HFr::zero();
  for (size_t s = 0; s < sets.size(); s++) {  // r_eval (kzg.rs:442-451)
    std::vector<HFr> pts;
    for (size_t i : sets[s].points) pts.push_back(points[i]);
    const std::vector<HFr> w = barycentric_weights(pts);
    HFr r = HFr::zero();
    for (size_t k = 0; k < sets[s].evals.size(); k++) r += pob[k] * barycentric_interpolate(w, pts, sets[s].evals[k], z);
    eval += sc.first[s] * r;
  }
  ukzg_verify(vp, host::g1_to_affine(f), z, eval, tr);
}

// ------------------------------------------------------------------ Gemini::{verify, batch_verify} (gemini.rs:165-211)
void gemini_verify(const UkzgVerifierParams& vp, const HG1& comm, const HFr* point, size_t num_vars, const HFr& eval,
                   Transcript& tr) {
  LH_REQUIRE(num_vars >= 1 && num_vars < 64, LH_ERR_ARG, "gemini verify: bad num_vars");
  std::vector<HG1> comms{comm};
  for (const HG1& p : tr.read_commitments(num_vars - 1)) comms.push_back(p);
  const HFr beta = tr.squeeze_challenge();
  std::vector<HFr> sq(num_vars);
  sq[0] = beta;
  for (size_t i = 1; i < num_vars; i++) sq[i] = sq[i - 1].sqr();
  const std::vector<HFr> evs = tr.read_field_elements(num_vars);
  const HFr one = HFr::one();
  HFr eval_0 = eval;
  for (size_t i = num_vars; i-- > 0;) {
    const HFr den = (one - point[i]) * sq[i] + point[i];
    LH_REQUIRE(!den.is_zero(), LH_ERR_INVALID_PCS_OPEN, "Invalid univariate KZG open");  // (the reference unwraps the inverse)
    eval_0 = (sq[i].dbl() * eval_0 - ((one - point[i]) * sq[i] - point[i]) * evs[i]) * den.inv();
  }
  std::vector<lh_evaluation> evals(num_vars + 1);
  auto set_eval = [&](size_t k, size_t poly, size_t pt, const HFr& v) {
    evals[k].poly = (uint32_t)poly, evals[k].point = (uint32_t)pt;
    memcpy(&evals[k].value, &v, 32);
  };
  set_eval(0, 0, 0, eval_0);
  set_eval(1, 0, 1, evs[0]);
  for (size_t i = 1; i < num_vars; i++) set_eval(i + 1, i, i + 1, evs[i]);
  std::vector<HFr> points(num_vars + 1);
  points[0] = beta;
  for (size_t i = 0; i < num_vars; i++) points[i + 1] = -sq[i];
  ukzg_batch_verify(vp, comms.data(), comms.size(), points.data(), points.size(), evals.data(), evals.size(), tr);
}
void gemini_batch_verify(const UkzgVerifierParams& vp, size_t num_vars, const HG1* comms, size_t num_comms, const HFr* points,
                         size_t num_points, const lh_evaluation* evals, size_t num_evals, Transcript& tr) {
  additive_batch_verify(num_vars, comms, num_comms, points, num_points, evals, num_evals, tr,
                        [&](const HG1& comm, const HFr* x, const HFr& eval) { gemini_verify(vp, comm, x, num_vars, eval, tr); });
}
PcsVerifier gemini_verifier(const UkzgVerifierParams& vp) {
  return {[&vp](auto&&... args) { gemini_batch_verify(vp, args...); }};
}

// ------------------------------------------------------------------ MultilinearIpa::{verify, batch_verify} (ipa.rs:269-337)
// variable_base_msm: the bucket method, one window per item of the host pool; only the affine sum is observable
HG1 host_msm(const HFr* scalars, const HG1* bases, size_t n) {
  if (!n) return HG1{host::Fq::zero(), host::Fq::zero()};
  size_t lg = 0;
  while (((size_t)2 << lg) <= n) lg++;
  const size_t c = std::min<size_t>(std::max<size_t>(lg > 2 ? lg - 2 : 1, 2), 13), windows = (254 + c - 1) / c;
  std::vector<uint64_t> canon(4 * n);
  for (size_t i = 0; i < n; i++) scalars[i].to_canonical(&canon[4 * i]);
  std::vector<host::G1Xyzz> sums(windows);
  host_parallel_for(windows, [&](size_t w) {
    std::vector<host::G1Xyzz> buckets(((size_t)1 << c) - 1, host::G1Xyzz::identity());
    const size_t bit = w * c;
    for (size_t i = 0; i < n; i++) {
      if (bases[i].is_identity()) continue;
      const uint64_t* k = &canon[4 * i];
      uint64_t d = k[bit >> 6] >> (bit & 63);
      if ((bit & 63) + c > 64 && (bit >> 6) < 3) d |= k[(bit >> 6) + 1] << (64 - (bit & 63));
      d &= ((uint64_t)1 << c) - 1;
      if (d) buckets[d - 1] = host::g1_add(buckets[d - 1], host::g1_from_affine(bases[i]));
    }
    host::G1Xyzz run = host::G1Xyzz::identity(), acc = host::G1Xyzz::identity();
    for (size_t b = buckets.size(); b-- > 0;) {
      run = host::g1_add(run, buckets[b]);
      acc = host::g1_add(acc, run);
    }
    sums[w] = acc;
  });
  host::G1Xyzz total = host::G1Xyzz::identity();
  for (size_t w = windows; w-- > 0;) {
    for (size_t k = 0; k < c; k++) total = host::g1_dbl(total);
    total = host::g1_add(total, sums[w]);
  }
  return host::g1_to_affine(total);
}

void ipa_verify(const IpaParams& vp, size_t poly_size, const HG1& comm, const HFr* point, size_t num_vars, const HFr& eval,
                Transcript& tr) {
  const size_t n = ipa_trim_vars(vp, poly_size);
  // (h_coeffs has 2^n entries for the PARAM's n and is evaluated at the point: the reference panics on any other length)
  LH_REQUIRE(num_vars == n, LH_ERR_ARG, "ipa verify: the point must have as many variables as the (trimmed) param");
  const std::vector<HG1>& g = ipa_host_g(vp);
  const HFr xi_0 = tr.squeeze_challenge();
  std::vector<HG1> bases(2 * n);
  std::vector<HFr> xis(n);
  for (size_t i = 0; i < n; i++) {
    bases[i] = tr.read_commitment();
    bases[n + i] = tr.read_commitment();
    xis[i] = tr.squeeze_challenge();
  }
  const HFr neg_c = -tr.read_field_element();
  std::vector<HFr> scalars(2 * n);
  {  // batch_invert (zeros stay zero, as ff's BatchInvert leaves them)
    std::vector<HFr> pre(n + 1);
    pre[0] = HFr::one();
    for (size_t i = 0; i < n; i++) pre[i + 1] = xis[i].is_zero() ? pre[i] : pre[i] * xis[i];
    HFr inv = pre[n].inv();
    for (size_t i = n; i-- > 0;) {
      if (xis[i].is_zero()) {
        scalars[i] = HFr::zero();
        continue;
      }
      scalars[i] = inv * pre[i];
      inv = inv * xis[i];
    }
  }
  for (size_t i = 0; i < n; i++) scalars[n + i] = xis[i];
  // h_coeffs (ipa.rs:319-337)
  const size_t size = (size_t)1 << n;
  std::vector<HFr> h(size);
  h[0] = neg_c;
  for (size_t i = 0, len = 1; i < n; i++, len <<= 1)
    for (size_t j = 0; j < len; j++) h[len + j] = h[j] * xis[n - 1 - i];
  std::vector<HFr> fold(h);  // neg_c_h.evaluate(point) (multilinear.rs:137-156)
  for (size_t i = 0, len = size >> 1; i < n; i++, len >>= 1)
    for (size_t j = 0; j < len; j++) fold[j] = fold[2 * j] + point[i] * (fold[2 * j + 1] - fold[2 * j]);
  const HFr u = xi_0 * (fold[0] + eval);
  scalars.insert(scalars.end(), h.begin(), h.end());
  bases.insert(bases.end(), g.begin(), g.begin() + size);
  scalars.push_back(u);
  bases.push_back(vp.h);
  const HG1 sum = host_msm(scalars.data(), bases.data(), scalars.size());
  if (!host::g1_add(host::g1_from_affine(sum), host::g1_from_affine(comm)).is_identity())
    throw Error(LH_ERR_INVALID_PCS_OPEN, "Invalid multilinear IPA open");
}
void ipa_batch_verify(const IpaParams& vp, size_t poly_size, size_t num_vars, const HG1* comms, size_t num_comms, const HFr* points,
                      size_t num_points, const lh_evaluation* evals, size_t num_evals, Transcript& tr) {
  additive_batch_verify(num_vars, comms, num_comms, points, num_points, evals, num_evals, tr, [&](const HG1& comm, const HFr* x, const HFr& eval) {
    ipa_verify(vp, poly_size, comm, x, num_vars, eval, tr);
  });
}
PcsVerifier ipa_verifier(const IpaParams& vp, size_t poly_size) {
  return {[&vp, poly_size](auto&&... args) { ipa_batch_verify(vp, poly_size, args...); }};
}

// ------------------------------------------------------------------ MultilinearHyrax::{verify, batch_verify} (hyrax.rs:288-320)
void hyrax_verify(const IpaParams& vp, size_t poly_size, size_t batch_size, const HG1* comm, const HFr* point, size_t num_vars,
                  const HFr& eval, Transcript& tr) {
  const HyraxDims d = hyrax_trim(vp, poly_size, batch_size);
  LH_REQUIRE(num_vars == d.num_vars, LH_ERR_ARG, "hyrax verify: the point must have as many variables as the (trimmed) param");
  const size_t chunks = d.num_chunks();
  HG1 row = comm[0];  // hi empty: the commitment is its single row (hyrax.rs:299-301)
  if (chunks > 1) {
    const std::vector<HFr> w = host_eq_xy(std::vector<HFr>(point + d.row_num_vars, point + num_vars));
    row = host_msm(w.data(), comm, chunks);
  }
  ipa_verify(vp, (size_t)1 << d.row_num_vars, row, point, d.row_num_vars, eval, tr);
}
void hyrax_batch_verify(const IpaParams& vp, size_t poly_size, size_t batch_size, size_t num_vars, const HG1* comms,
                        size_t num_comms, const HFr* points, size_t num_points, const lh_evaluation* evals, size_t num_evals,
                        Transcript& tr) {
  const HyraxDims d = hyrax_trim(vp, poly_size, batch_size);
  LH_REQUIRE(num_vars == d.num_vars, LH_ERR_ARG, "hyrax batch verify: num_vars differs from the (trimmed) param's");
  additive_batch_verify_chunks(num_vars, comms, num_comms, d.num_chunks(), points, num_points, evals, num_evals, tr,
                               [&](const HG1* comm, const HFr* x, const HFr& eval) {
                                 hyrax_verify(vp, poly_size, batch_size, comm, x, num_vars, eval, tr);
                               });
}
PcsVerifier hyrax_verifier(const IpaParams& vp, size_t poly_size, size_t batch_size) {
  const size_t chunks = hyrax_trim(vp, poly_size, batch_size).num_chunks();
  return {[&vp, poly_size, batch_size](auto&&... args) { hyrax_batch_verify(vp, poly_size, batch_size, args...); }, chunks};
}

// ------------------------------------------------------------------ expressions on the host
static void check_expr(const lh_expr& e) {
  LH_REQUIRE(e.nodes && e.num_nodes, LH_ERR_ARG, "empty expression");
  for (size_t i = 0; i < e.num_nodes; i++) {
    const lh_expr_node& nd = e.nodes[i];
    LH_REQUIRE(nd.op <= LH_EX_SCALED, LH_ERR_ARG, "expression: bad op");
    if (nd.op >= LH_EX_NEGATED) LH_REQUIRE(nd.a >= 0 && (size_t)nd.a < i, LH_ERR_ARG, "expression: bad child");
    if (nd.op == LH_EX_SUM || nd.op == LH_EX_PRODUCT)
      LH_REQUIRE(nd.b >= 0 && (size_t)nd.b < i, LH_ERR_ARG, "expression: bad child");
  }
}
static size_t expr_degree(const lh_expr& e) {  // expression.rs:171-182
  std::vector<size_t> d(e.num_nodes);
  for (size_t i = 0; i < e.num_nodes; i++) {
    const lh_expr_node& nd = e.nodes[i];
    switch (nd.op) {
      case LH_EX_CONSTANT:
      case LH_EX_CHALLENGE: d[i] = 0; break;
      case LH_EX_NEGATED:
      case LH_EX_SCALED: d[i] = d[nd.a]; break;
      case LH_EX_SUM: d[i] = std::max(d[nd.a], d[nd.b]); break;
      case LH_EX_PRODUCT: d[i] = d[nd.a] + d[nd.b]; break;
      default: d[i] = 1;
    }
  }
  return d.back();
}
struct EvalCtx {
  HFr identity;
  std::map<int, HFr> lagrange;
  std::vector<HFr> eq_xys;
  std::map<std::pair<size_t, int>, HFr> evals;
  std::vector<HFr> challenges;
};
static HFr eval_expr(const lh_expr& e, const EvalCtx& cx) {  // piop/sum_check.rs:60-98
  std::vector<HFr> v(e.num_nodes);
  for (size_t i = 0; i < e.num_nodes; i++) {
    const lh_expr_node& nd = e.nodes[i];
    HFr sc;
    memcpy(&sc, &nd.scalar, 32);
    switch (nd.op) {
      case LH_EX_CONSTANT: v[i] = sc; break;
      case LH_EX_IDENTITY: v[i] = cx.identity; break;
      case LH_EX_LAGRANGE: v[i] = cx.lagrange.at(nd.a); break;
      case LH_EX_EQ_XY:
        LH_REQUIRE(nd.a >= 0 && (size_t)nd.a < cx.eq_xys.size(), LH_ERR_ARG, "expression: eq_xy index");
        v[i] = cx.eq_xys[nd.a];
        break;
      case LH_EX_POLYNOMIAL: {
        auto it = cx.evals.find({(size_t)nd.a, nd.b});
        LH_REQUIRE(it != cx.evals.end(), LH_ERR_ARG, "expression: query without evaluation");
        v[i] = it->second;
        break;
      }
      case LH_EX_CHALLENGE:
        LH_REQUIRE(nd.a >= 0 && (size_t)nd.a < cx.challenges.size(), LH_ERR_ARG, "expression: challenge index");
        v[i] = cx.challenges[nd.a];
        break;
      case LH_EX_NEGATED: v[i] = -v[nd.a]; break;
      case LH_EX_SUM: v[i] = v[nd.a] + v[nd.b]; break;
      case LH_EX_PRODUCT: v[i] = v[nd.a] * v[nd.b]; break;
      default: v[i] = v[nd.a] * sc;
    }
  }
  return v.back();
}

HFr identity_eval(const std::vector<HFr>& x) {  // sum_check.rs:123-125
  HFr acc = HFr::zero(), p = HFr::one();
  for (auto& xi : x) {
    acc += xi * p;
    p = p.dbl();
  }
  return acc;
}
static HFr lagrange_eval(const std::vector<HFr>& x, size_t b) {  // sum_check.rs:100-111
  HFr acc = HFr::one();
  for (size_t i = 0; i < x.size(); i++) acc *= ((b >> i) & 1) ? x[i] : HFr::one() - x[i];
  return acc;
}
// the row of BooleanHypercube::iter() at position i.rem_euclid(2^num_vars)
static size_t bh_row(size_t num_vars, long long i) {
  const long long n = (long long)1 << num_vars;
  long long m = i % n;
  if (m < 0) m += n;
  return bh_nth(num_vars, (size_t)m);
}

// poly/multilinear.rs:435-475,528-549
static std::vector<size_t> coeff_pattern(bool next, size_t num_vars, size_t distance) {
  const size_t rem = next ? (size_t)bh_primitive(num_vars) - ((size_t)1 << num_vars) : (size_t)bh_x_inv(num_vars) << distance;
  std::vector<size_t> pat((size_t)1 << (distance - 1), 0);
  for (size_t depth = 0; depth + 1 < distance; depth++) {
    size_t step = (size_t)1 << (distance - depth - 1);
    for (size_t e = 0; e < pat.size(); e += step) {
      size_t o = e + step / 2;
      size_t rot = next ? pat[e] << 1 : pat[e] >> 1;
      pat[o] = rot ^ rem;
      pat[e] = rot;
    }
  }
  return pat;
}
static HFr rotation_eval(const std::vector<HFr>& x, int rotation, const std::vector<HFr>& evals_for_rotation) {
  if (rotation == 0) return evals_for_rotation[0];
  const size_t n = x.size(), distance = (size_t)std::abs(rotation);
  LH_REQUIRE(distance <= n && evals_for_rotation.size() == ((size_t)1 << distance), LH_ERR_ARG, "rotation_eval: shape");
  std::vector<size_t> pat = coeff_pattern(rotation > 0, n, distance), nths(distance);
  std::vector<HFr> xs(distance);
  for (size_t i = 0; i < distance; i++) {
    if (rotation < 0) {
      nths[i] = distance - i;
      xs[i] = x[distance - 1 - i];
    } else {
      nths[i] = n - 1 + i;
      xs[i] = x[n - distance + i];
    }
  }
  std::vector<HFr> evals = evals_for_rotation;
  for (size_t idx = 0; idx < distance; idx++) {
    std::vector<HFr> next(evals.size() / 2);
    for (size_t k = 0; k < next.size(); k++) {
      const bool flip = (pat[k << idx] >> nths[idx]) & 1;
      const HFr &e0 = evals[2 * k], &e1 = evals[2 * k + 1];
      next[k] = flip ? (e0 - e1) * xs[idx] + e1 : (e1 - e0) * xs[idx] + e0;
    }
    evals.swap(next);
  }
  return evals[0];
}

// ------------------------------------------------------------------ HyperPlonk::verify
static void lasso_verify_check_table(const lh_lasso_table& tb, size_t n);

void hyperplonk_verify(const PcsVerifier& pcs, const lh_hp_vparam& vp, const HFr* const* instances, Transcript& tr) {
  hyperplonk_verify_phases(pcs, vp, {vp.num_witness_polys}, {vp.num_challenges}, instances, tr);
}

void hyperplonk_verify_phases(const PcsVerifier& pcs, const lh_hp_vparam& vp, const std::vector<size_t>& phase_witness_polys,
                              const std::vector<size_t>& phase_challenges, const HFr* const* instances, Transcript& tr) {
  const size_t chunks = pcs.chunks;
  auto read_comms = [&](size_t count) { return pcs.read_commitments ? pcs.read_commitments(tr, count) : tr.read_commitments(count); };
  LH_REQUIRE(!pcs.read_commitments || vp.num_lasso_lookups == 0, LH_ERR_ARG,
             "hyperplonk: Lasso lookups need a PCS that commits to points");
  // chunks: points per commitment (Hyrax's rows; 1 otherwise) - every commitment is read as that many points, the verifier
  // param holds that many per poly, and batch_verify gets the commitments as vectors, commitment-major
  LH_REQUIRE(chunks >= 1, LH_ERR_ARG, "hyperplonk: chunks must be at least 1");
  const size_t nv = vp.num_vars;
  LH_REQUIRE(phase_witness_polys.size() == phase_challenges.size(), LH_ERR_ARG, "hyperplonk: phases are malformed");
  {
    size_t w = 0, ch = 0;
    for (size_t v : phase_witness_polys) w += v;
    for (size_t v : phase_challenges) ch += v;
    LH_REQUIRE(w == vp.num_witness_polys && ch == vp.num_challenges, LH_ERR_ARG,
               "hyperplonk: phases do not add up to num_witness_polys / num_challenges");
  }
  LH_REQUIRE(nv >= 1 && nv < 32, LH_ERR_ARG, "hyperplonk: bad num_vars");
  check_expr(vp.expression);
  for (size_t i = 0; i < vp.num_instance_polys; i++)
    for (size_t k = 0; k < vp.num_instances[i]; k++) tr.common_field_element(instances[i][k]);
  // rounds 0..n (hyperplonk.rs:309-316): per phase read the witness commitments, squeeze the phase's challenges
  std::vector<HG1> witness_comms;
  std::vector<HFr> challenges;
  for (size_t r = 0; r < phase_witness_polys.size(); r++) {
    std::vector<HG1> cm = read_comms(phase_witness_polys[r] * chunks);
    witness_comms.insert(witness_comms.end(), cm.begin(), cm.end());
    std::vector<HFr> ch = tr.squeeze_challenges(phase_challenges[r]);
    challenges.insert(challenges.end(), ch.begin(), ch.end());
  }
  HFr beta = tr.squeeze_challenge();
  std::vector<HG1> m_comms = read_comms(vp.num_lookups * chunks);
  // Lasso lookups (oracle/pyref/hyperplonk.py LassoLookup): read_ts | E | final_cts per lookup, identity-mask framing
  std::vector<HG1> lasso_comms;
  if (vp.num_lasso_lookups) {
    LH_REQUIRE(vp.lasso_lookups != nullptr, LH_ERR_ARG, "hyperplonk: lasso_lookups is null");
    size_t count = 0;
    for (size_t k = 0; k < vp.num_lasso_lookups; k++) {
      const lh_hp_lasso_lookup& lk = vp.lasso_lookups[k];
      lasso_verify_check_table(lk.table, nv);
      if (lk.table.chunk_bits > nv) throw Error(LH_ERR_INVALID_SNARK, "Lasso subtable larger than the circuit");
      count += LassoOpening::circuit_polys(LassoLayout(lk.table));
    }
    lasso_comms = lasso_read_commitments(tr, count, chunks);
  }
  HFr gamma = tr.squeeze_challenge();
  std::vector<HG1> hz_comms = read_comms((vp.num_lookups + vp.num_permutation_z_polys) * chunks);
  HFr alpha = tr.squeeze_challenge();
  std::vector<HFr> y = tr.squeeze_challenges(nv);
  challenges.push_back(beta);
  challenges.push_back(gamma);
  challenges.push_back(alpha);

  // verify_sum_check (verifier.rs:39-90), zero-check: sum = 0
  auto res = sum_check_verify(LH_SC_EVALUATIONS, nv, expr_degree(vp.expression), HFr::zero(), tr);
  const std::vector<HFr>& x = res.second;
  std::set<std::pair<size_t, int>> pcs_query, inst_query;
  std::set<int> lag_used;
  for (size_t i = 0; i < vp.expression.num_nodes; i++) {
    const lh_expr_node& nd = vp.expression.nodes[i];
    if (nd.op == LH_EX_POLYNOMIAL) {
      LH_REQUIRE(nd.a >= 0 && (size_t)std::abs(nd.b) <= nv, LH_ERR_ARG, "expression: bad query");
      ((size_t)nd.a >= vp.num_instance_polys ? pcs_query : inst_query).insert({(size_t)nd.a, nd.b});
    } else if (nd.op == LH_EX_LAGRANGE) {
      lag_used.insert(nd.a);
    }
  }
  EvalCtx cx;
  std::vector<std::vector<HFr>> evals_for_rotation;
  for (auto& q : pcs_query) {
    evals_for_rotation.push_back(tr.read_field_elements((size_t)1 << std::abs(q.second)));
    cx.evals[q] = rotation_eval(x, q.second, evals_for_rotation.back());
  }
  {  // instance_evals (verifier.rs:92-145): instance polys are known to the verifier through Lagrange evals
    long long lo = 0, hi = 0;
    for (auto& q : inst_query) {
      long long i = -(long long)q.second;
      lo = std::min(lo, i);
      hi = std::max(hi, i + (long long)vp.num_instances[q.first]);
    }
    if (lo < 0) lo -= 1;
    if (hi > 0) hi += 1;
    std::map<long long, HFr> lag;
    for (long long i = lo; i < hi; i++)
      if (i != 0) lag[i] = lagrange_eval(x, bh_row(nv, i));
    for (auto& q : inst_query) {
      const long long cnt = (long long)vp.num_instances[q.first], rot = q.second;
      std::vector<long long> idxs;
      if (rot > 0) {
        for (long long i = -rot; i < 0; i++) idxs.push_back(i);
        for (long long i = 1; i <= cnt; i++) idxs.push_back(i);
        idxs.resize((size_t)cnt);
      } else {
        for (long long i = 1 - rot; i < 1 - rot + cnt; i++) idxs.push_back(i);
      }
      HFr acc = HFr::zero();
      for (long long k = 0; k < cnt; k++) acc += instances[q.first][k] * lag.at(idxs[(size_t)k]);
      cx.evals[q] = acc;
    }
  }
  cx.identity = identity_eval(x);
  for (int i : lag_used) cx.lagrange[i] = lagrange_eval(x, bh_row(nv, i));
  cx.eq_xys.push_back(host_eq_xy_eval(x.data(), y.data(), nv));
  cx.challenges = challenges;
  if (eval_expr(vp.expression, cx) != res.first)
    throw Error(LH_ERR_INVALID_SNARK, "Unmatched between sum_check output and query evaluation");

  // points / evaluations in pcs_query order (verifier.rs:76-89,147-180)
  std::set<int> rots;
  for (auto& q : pcs_query) rots.insert(q.second);
  std::map<int, size_t> point_off;
  std::vector<HFr> points;
  size_t num_points = 0;
  for (int r : rots) {
    point_off[r] = num_points;
    for (auto& pt : rotation_eval_points(x, r)) {
      points.insert(points.end(), pt.begin(), pt.end());
      num_points++;
    }
  }
  std::vector<lh_evaluation> evals;
  size_t qi = 0;
  for (auto& q : pcs_query) {
    const std::vector<HFr>& efr = evals_for_rotation[qi++];
    for (size_t k = 0; k < efr.size(); k++) {
      lh_evaluation e;
      e.poly = (uint32_t)q.first;
      e.point = (uint32_t)(point_off[q.second] + k);
      memcpy(&e.value, &efr[k], 32);
      evals.push_back(e);
    }
  }
  std::vector<HG1> comms(vp.num_instance_polys * chunks, HG1{host::Fq::zero(), host::Fq::zero()});  // Commitment::default()
  for (size_t i = 0; i < vp.num_preprocess_polys * chunks; i++) {
    HG1 p;
    memcpy(&p, &vp.preprocess_comms[i], sizeof(p));
    comms.push_back(p);
  }
  comms.insert(comms.end(), witness_comms.begin(), witness_comms.end());
  for (size_t i = 0; i < vp.num_permutation_polys * chunks; i++) {
    HG1 p;
    memcpy(&p, &vp.permutation_comms[i], sizeof(p));
    comms.push_back(p);
  }
  comms.insert(comms.end(), m_comms.begin(), m_comms.end());
  comms.insert(comms.end(), hz_comms.begin(), hz_comms.end());
  // Lasso lookups: the argument's checks, then its claims join the one batch verification
  size_t base = comms.size() / chunks;  // (poly indices count commitments, not points)
  comms.insert(comms.end(), lasso_comms.begin(), lasso_comms.end());
  for (size_t k = 0; k < vp.num_lasso_lookups; k++) {
    const lh_hp_lasso_lookup& lk = vp.lasso_lookups[k];
    const lh_lasso_table& tb = lk.table;
    const LassoLayout lay(tb);
    const size_t cc = lay.cc, l = lay.l, alpha = lay.alpha;
    // the prover's range (hyperplonk.cpp): preprocess and witness polys - instance polys have no commitment to open, the
    // polys after the witness do not exist yet when the lookup's columns are read
    const size_t first_committed = vp.num_instance_polys;
    const size_t end_committed = vp.num_instance_polys + vp.num_preprocess_polys + witness_comms.size() / chunks;
    LH_REQUIRE(lk.output_poly >= first_committed && lk.output_poly < end_committed, LH_ERR_ARG, "hyperplonk: lasso output poly out of range");
    for (size_t j = 0; j < cc; j++)
      LH_REQUIRE(lk.chunk_polys[j] >= first_committed && lk.chunk_polys[j] < end_committed, LH_ERR_ARG,
                 "hyperplonk: lasso chunk poly out of range");
    for (size_t v : {nv, l, cc, alpha}) tr.common_field_element(HFr::from_u64(v));
    LassoClaims cl = lasso_check(tb, nv, tr);
    const size_t p0 = num_points;
    lasso_append_points(points, {&cl.r, &cl.r_z, &cl.r_N, &cl.r_M}, nv);
    num_points += 4;
    lasso_evaluation_list(lay, LassoOpening::in_circuit(lay, lk.output_poly, lk.chunk_polys, base, p0), &cl, evals);
    base += LassoOpening::circuit_polys(lay);
  }
  pcs.batch_verify(nv, comms.data(), comms.size() / chunks, points.data(), num_points, evals.data(), evals.size(), tr);
}

// ------------------------------------------------------------------ Lasso verify (oracle/pyref/lasso.py:219-261)
// oracle/pyref/gkr.py:197-227 (layer schedule of fractional_sum_check.rs:193-270 with p dropped; GpClaim: host.hpp)
std::vector<HFr> verify_grand_product(const std::vector<size_t>& depth, Transcript& tr, std::vector<GpClaim>& out) {
  const size_t B = depth.size();
  size_t max_depth = 0;
  for (size_t d : depth) max_depth = std::max(max_depth, d);
  std::vector<HFr> roots = tr.read_field_elements(B), claims = roots, y;
  out.assign(B, GpClaim());
  for (size_t h = 0; h < max_depth; h++) {
    std::vector<size_t> active;
    for (size_t b = 0; b < B; b++)
      if (depth[b] > h) active.push_back(b);
    std::vector<HFr> evals, x;
    if (h == 0) {
      evals = tr.read_field_elements(2 * active.size());
      for (size_t k = 0; k < active.size(); k++)
        if (claims[active[k]] != evals[2 * k] * evals[2 * k + 1])
          throw Error(LH_ERR_INVALID_SUMCHECK, "grand product: root mismatch");
    } else {
      HFr lam = tr.squeeze_challenge(), claim = HFr::zero(), power = HFr::one();
      for (size_t b : active) {
        claim += claims[b] * power;
        power *= lam;
      }
      auto res = sum_check_verify(LH_SC_EVALUATIONS, h, 3, claim, tr);
      x = res.second;
      evals = tr.read_field_elements(2 * active.size());
      HFr acc = HFr::zero();
      power = HFr::one();
      for (size_t k = 0; k < active.size(); k++) {
        acc += evals[2 * k] * evals[2 * k + 1] * power;
        power *= lam;
      }
      if (res.first != acc * host_eq_xy_eval(x.data(), y.data(), h))
        throw Error(LH_ERR_INVALID_SUMCHECK, "grand product: layer " + std::to_string(h) + " mismatch");
    }
    HFr mu = tr.squeeze_challenge();
    y = x;
    y.push_back(mu);
    for (size_t k = 0; k < active.size(); k++) {
      const size_t b = active[k];
      claims[b] = evals[2 * k] + mu * (evals[2 * k + 1] - evals[2 * k]);
      if (depth[b] == h + 1) out[b] = GpClaim{claims[b], y};
    }
  }
  return roots;
}

// fractional_sum_check.rs:193-270 (oracle/pyref/gkr.py verify_fractional_sum_check), the roots returned with the rest
FracVerifyResult verify_fractional_sum_check(size_t B, size_t num_vars, const HFr* const* claimed_p_0s,
                                             const HFr* const* claimed_q_0s, Transcript& tr) {
  LH_REQUIRE(B != 0, LH_ERR_ARG, "fractional sum-check: num_batching == 0");
  LH_REQUIRE(num_vars >= 1 && num_vars < 64, LH_ERR_ARG, "fractional sum-check: num_vars out of range");
  LH_REQUIRE(3 * B <= LH_SC_MAX_TERMS, LH_ERR_ARG, "fractional sum-check: more fractions than the prover's layer sum-check takes");
  FracVerifyResult res;
  for (int side = 0; side < 2; side++) {  // :207-222: Some -> common, None -> read
    const HFr* const* claimed = side ? claimed_q_0s : claimed_p_0s;
    std::vector<HFr>& roots = side ? res.q_0s : res.p_0s;
    for (size_t b = 0; b < B; b++) {
      if (claimed && claimed[b]) {
        tr.common_field_element(*claimed[b]);
        roots.push_back(*claimed[b]);
      } else {
        roots.push_back(tr.read_field_element());
      }
    }
  }
  std::vector<HFr> claimed_p = res.p_0s, claimed_q = res.q_0s, y;
  const char* const mismatch = "Unmatched between sum_check output and query evaluation";
  for (size_t nv = 0; nv < num_vars; nv++) {
    std::vector<HFr> x, evals;
    if (nv == 0) {
      evals = tr.read_field_elements(4 * B);
      for (size_t b = 0; b < B; b++) {
        const HFr &p_l = evals[4 * b], &p_r = evals[4 * b + 1], &q_l = evals[4 * b + 2], &q_r = evals[4 * b + 3];
        if (claimed_p[b] != p_l * q_r + p_r * q_l || claimed_q[b] != q_l * q_r) throw Error(LH_ERR_INVALID_SUMCHECK, mismatch);
      }
    } else {
      const HFr gamma = tr.squeeze_challenge();
      HFr claim = HFr::zero(), power = HFr::one();
      for (size_t b = 0; b < B; b++) {  // sum_check_claim (:283-288)
        claim += claimed_p[b] * power;
        power *= gamma;
        claim += claimed_q[b] * power;
        power *= gamma;
      }
      auto sc = sum_check_verify(LH_SC_EVALUATIONS, nv, 3, claim, tr);
      x = sc.second;
      evals = tr.read_field_elements(4 * B);
      HFr acc = HFr::zero();  // sum_check_expression (:272-281) at the evaluations
      power = HFr::one();
      for (size_t b = 0; b < B; b++) {
        const HFr &p_l = evals[4 * b], &p_r = evals[4 * b + 1], &q_l = evals[4 * b + 2], &q_r = evals[4 * b + 3];
        acc += (p_l * q_r + p_r * q_l) * power;
        power *= gamma;
        acc += q_l * q_r * power;
        power *= gamma;
      }
      if (sc.first != acc * host_eq_xy_eval(x.data(), y.data(), nv)) throw Error(LH_ERR_INVALID_SUMCHECK, mismatch);
    }
    const HFr mu = tr.squeeze_challenge();
    for (size_t b = 0; b < B; b++) {  // layer_down_claim (:290-296)
      const HFr &p_l = evals[4 * b], &p_r = evals[4 * b + 1], &q_l = evals[4 * b + 2], &q_r = evals[4 * b + 3];
      claimed_p[b] = p_l + mu * (p_r - p_l);
      claimed_q[b] = q_l + mu * (q_r - q_l);
    }
    x.push_back(mu);
    y = x;
  }
  res.p_xs = claimed_p, res.q_xs = claimed_q, res.x = y;
  return res;
}

static HFr subtable_mle_eval(uint32_t kind, const std::vector<HFr>& point) {  // lasso.py:55-72
  if (subtable_is_custom(kind)) {
    // a registered subtable: the dense MLE of its entries, one fold over 2^l values (variable i = index bit i); the fold of
    // the first variable reads the 32-bit entries
    const std::shared_ptr<const CustomSubtable> t = subtable_require(kind, point.size());
    const std::vector<uint32_t>& T = t->values;
    std::vector<HFr> cur(T.size() / 2);
    for (size_t k = 0; k < cur.size(); k++) {
      const HFr lo = HFr::from_u64(T[2 * k]), hi = HFr::from_u64(T[2 * k + 1]);
      cur[k] = lo + point[0] * (hi - lo);
    }
    for (size_t i = 1; i < point.size(); i++) {
      const size_t half = cur.size() / 2;
      for (size_t k = 0; k < half; k++) cur[k] = cur[2 * k] + point[i] * (cur[2 * k + 1] - cur[2 * k]);
      cur.resize(half);
    }
    return cur[0];
  }
  if (kind == LH_SUBTABLE_IDENTITY) return identity_eval(point);
  const size_t h = point.size() / 2;
  if (kind == LH_SUBTABLE_EQ || kind == LH_SUBTABLE_LTU) {
    // e_i = x_i y_i + (1 - x_i)(1 - y_i);  EQ = prod_i e_i;  LTU = sum_i (1 - x_i) y_i prod_{k > i} e_k (the high bits
    // decide first): from the top bit down, `eq` is the product of the e_k above bit i
    HFr eq = HFr::one(), lt = HFr::zero();
    for (size_t i = h; i-- > 0;) {
      const HFr &yi = point[i], &xi = point[h + i];
      const HFr xy = xi * yi;
      lt += (yi - xy) * eq;
      eq *= xy.dbl() + HFr::one() - xi - yi;
    }
    return kind == LH_SUBTABLE_EQ ? eq : lt;
  }
  HFr acc = HFr::zero(), p = HFr::one();
  for (size_t i = 0; i < h; i++) {
    const HFr &yi = point[i], &xi = point[h + i];
    HFr xy = xi * yi;
    acc += (kind == LH_SUBTABLE_AND ? xy : kind == LH_SUBTABLE_OR ? xi + yi - xy : xi + yi - xy.dbl()) * p;
    p = p.dbl();
  }
  return acc;
}

static void lasso_verify_check_table(const lh_lasso_table& tb, size_t n) {
  const size_t c = tb.num_chunks, l = tb.chunk_bits, alpha = tb.num_memories;
  LH_REQUIRE(c >= 1 && c <= LH_LASSO_MAX_CHUNKS && alpha >= 1 && alpha <= LH_LASSO_MAX_MEMORIES &&
                 tb.num_terms <= LH_LASSO_MAX_TERMS,
             LH_ERR_ARG, "lasso: bad table");
  LH_REQUIRE(n >= 1 && l >= 1 && n < 32 && l < 32, LH_ERR_ARG, "lasso: need at least one variable");
  for (size_t i = 0; i < alpha; i++) {
    if (tb.memory_chunk[i] < c && subtable_is_custom(tb.memory_subtable[i])) {  // (registered, and of this table's size)
      subtable_require(tb.memory_subtable[i], l);
      continue;
    }
    LH_REQUIRE(tb.memory_chunk[i] < c && tb.memory_subtable[i] < LH_SUBTABLE_KINDS, LH_ERR_ARG, "lasso: bad memory");
  }
  LH_REQUIRE(tb.num_terms >= 1, LH_ERR_ARG, "lasso: bad g term count");
  for (size_t m = 0; m < tb.num_terms; m++)
    LH_REQUIRE(tb.g_num_factors[m] >= 1 && tb.g_num_factors[m] <= LH_SC_MAX_FACTORS, LH_ERR_ARG, "lasso: bad g term");
}

// the verifier's side of lasso_argue, over K tables that share r, gamma and tau, one Surge sum-check and one grand product
// (oracle/pyref/lasso.py check for K = 1, tests/lasso_batch_ref.py verify with `squeeze_rho`: then rho is squeezed behind the
// a_t(r) and table t's g counts rho^t; without it the one table counts once).  Reads the messages, checks Surge and the
// memory-checking identities table by table, returns every table's points and claimed evaluations left to check against
// the commitments: r, r_z, r_N are the same for all, r_M for all of one chunk size.
static std::vector<LassoClaims> lasso_check_tables(const lh_lasso_table* const* tables, size_t K, size_t n, bool squeeze_rho,
                                                   Transcript& tr) {
  std::vector<LassoLayout> lay(K);
  std::vector<size_t> mem_base(K);
  size_t A = 0, g_degree = 0;
  for (size_t t = 0; t < K; t++) {
    lay[t] = LassoLayout(*tables[t]);
    mem_base[t] = A, A += lay[t].alpha;
    g_degree = std::max(g_degree, lay[t].g_degree);
  }
  std::vector<LassoClaims> cls(K);
  const std::vector<HFr> r = tr.squeeze_challenges(n);
  for (LassoClaims& cl : cls) cl.v = tr.read_field_element();
  const HFr rho = squeeze_rho ? tr.squeeze_challenge() : HFr::one();
  HFr claim = HFr::zero(), power = HFr::one();
  for (size_t t = 0; t < K; t++) {
    claim += power * cls[t].v;
    power *= rho;
  }
  auto surge = sum_check_verify(LH_SC_EVALUATIONS, n, g_degree + 1, claim, tr);
  const std::vector<HFr>& r_z = surge.second;
  HFr want = HFr::zero();
  power = HFr::one();
  for (size_t t = 0; t < K; t++) cls[t].e_rz = tr.read_field_elements(lay[t].alpha);
  for (size_t t = 0; t < K; t++) {
    const lh_lasso_table& tb = *tables[t];
    HFr acc = HFr::zero();
    for (size_t m = 0; m < tb.num_terms; m++) {
      HFr term = lasso_g_coeff(tb, m);
      for (size_t k = 0; k < tb.g_num_factors[m]; k++) {
        LH_REQUIRE(tb.g_factor[m][k] < lay[t].alpha, LH_ERR_ARG, "lasso: bad g factor");
        term *= cls[t].e_rz[tb.g_factor[m][k]];
      }
      acc += term;
    }
    want += power * acc;
    power *= rho;
  }
  if (surge.first != host_eq_xy_eval(r_z.data(), r.data(), n) * want)
    throw Error(LH_ERR_INVALID_SNARK, "Surge sum-check final evaluation mismatch");

  // the n-variable trees RS, WS of every memory, then Init, Final of every memory
  const HFr gamma = tr.squeeze_challenge(), tau = tr.squeeze_challenge();
  std::vector<size_t> depth(2 * A, n);
  for (size_t t = 0; t < K; t++) depth.insert(depth.end(), 2 * lay[t].alpha, lay[t].l);
  std::vector<GpClaim> claims;
  const std::vector<HFr> roots = verify_grand_product(depth, tr, claims);
  const HFr *rw = roots.data(), *inf = roots.data() + 2 * A;  // (RS, WS) and (Init, Final) of memory b at [2 b], [2 b + 1]
  for (size_t b = 0; b < A; b++)
    if (inf[2 * b] * rw[2 * b + 1] != rw[2 * b] * inf[2 * b + 1])
      throw Error(LH_ERR_INVALID_SNARK, "memory " + std::to_string(b) + ": Init*WS != RS*Final");

  const Fingerprint fingerprint{gamma, tau};
  const HFr one = HFr::one();
  const GpClaim *rw_c = claims.data(), *inf_c = claims.data() + 2 * A;
  for (size_t t = 0; t < K; t++) {
    const lh_lasso_table& tb = *tables[t];
    LassoClaims& cl = cls[t];
    cl.r = r, cl.r_z = r_z, cl.r_N = rw_c[0].point, cl.r_M = inf_c[2 * mem_base[t]].point;
    cl.ev_n = tr.read_field_elements(lay[t].num_at_n());
    cl.ev_l = tr.read_field_elements(lay[t].cc);
    const HFr *dim_e = cl.ev_n.data(), *rts_e = dim_e + lay[t].cc, *e_e = rts_e + lay[t].cc, *fc_e = cl.ev_l.data();
    const HFr id_M = identity_eval(cl.r_M);
    for (size_t i = 0; i < lay[t].alpha; i++) {
      const size_t j = tb.memory_chunk[i], b = mem_base[t] + i;
      const HFr rs = fingerprint(dim_e[j], e_e[i], rts_e[j]);
      const HFr init = fingerprint(id_M, subtable_mle_eval(tb.memory_subtable[i], cl.r_M), HFr::zero());
      if (rw_c[2 * b].claim != rs || rw_c[2 * b + 1].claim != rs + one || inf_c[2 * b].claim != init ||
          inf_c[2 * b + 1].claim != init + fc_e[j])
        throw Error(LH_ERR_INVALID_SNARK, "memory " + std::to_string(b) + ": leaf claim mismatch");
    }
  }
  return cls;
}
LassoClaims lasso_check(const lh_lasso_table& tb, size_t n, Transcript& tr) {
  const lh_lasso_table* one = &tb;
  return lasso_check_tables(&one, 1, n, false, tr)[0];
}

void lasso_verify(const PcsVerifier& pcs, const lh_lasso_table& tb, size_t n, Transcript& tr) {
  const size_t chunks = pcs.chunks;
  lasso_verify_check_table(tb, n);
  const LassoLayout lay(tb);
  for (size_t v : {n, lay.l, lay.cc, lay.alpha}) tr.common_field_element(HFr::from_u64(v));
  const size_t nv = std::max(n, lay.l);
  std::vector<HG1> comms;
  if (pcs.read_commitments) {
    // commitments that are no points (Brakedown's roots): none of them can be the identity, so the mask element is zero
    if (!tr.read_field_element().is_zero()) throw Error(LH_ERR_INVALID_SNARK, "lasso: commitment mask out of range");
    comms = pcs.read_commitments(tr, lay.num_polys());
  } else {
    comms = lasso_read_commitments(tr, lay.num_polys(), chunks);
  }
  const LassoClaims cl = lasso_check(tb, n, tr);
  std::vector<lh_evaluation> evals;
  lasso_evaluation_list(lay, LassoOpening::block(lay), &cl, evals);
  std::vector<HFr> points;
  lasso_append_points(points, {&cl.r, &cl.r_z, &cl.r_N, &cl.r_M}, nv);
  pcs.batch_verify(nv, comms.data(), comms.size() / chunks, points.data(), 4, evals.data(), evals.size(), tr);
}

// the verifier of lasso_prove_batch (tests/lasso_batch_ref.py verify): its header and block-wise commitments, the argument's
// checks over the K tables with rho, one batch opening; r_M of the q-th distinct chunk size is point 3 + q
static void lasso_verify_batch_checked(const PcsVerifier& pcs, const lh_lasso_table* const* tables, size_t K, size_t n, size_t nv,
                                       Transcript& tr) {
  std::vector<LassoLayout> lay(K);
  for (size_t t = 0; t < K; t++) lay[t] = LassoLayout(*tables[t]);
  tr.common_field_element(HFr::from_u64(K));
  tr.common_field_element(HFr::from_u64(n));
  for (size_t t = 0; t < K; t++)
    for (size_t v : {lay[t].l, lay[t].cc, lay[t].alpha}) tr.common_field_element(HFr::from_u64(v));
  std::vector<HG1> comms;
  for (size_t t = 0; t < K; t++) {
    std::vector<HG1> block = lasso_read_commitments(tr, lay[t].num_polys());
    comms.insert(comms.end(), block.begin(), block.end());
  }
  const std::vector<LassoClaims> cls = lasso_check_tables(tables, K, n, true, tr);
  std::vector<const std::vector<HFr>*> pts = {&cls[0].r, &cls[0].r_z, &cls[0].r_N};
  std::vector<size_t> ls;  // the distinct chunk sizes in order of first appearance
  std::vector<lh_evaluation> evals;
  size_t poly_base = 0;
  for (size_t t = 0; t < K; t++) {
    const size_t q = (size_t)(std::find(ls.begin(), ls.end(), lay[t].l) - ls.begin());
    if (q == ls.size()) ls.push_back(lay[t].l), pts.push_back(&cls[t].r_M);
    lasso_evaluation_list(lay[t], LassoOpening::block(lay[t], poly_base, 3 + q), &cls[t], evals);
    poly_base += lay[t].num_polys();
  }
  std::vector<HFr> points;
  lasso_append_points(points, pts, nv);
  pcs.batch_verify(nv, comms.data(), comms.size(), points.data(), pts.size(), evals.data(), evals.size(), tr);
}
void lasso_verify_batch(const PcsVerifier& pcs, const lh_lasso_table* const* tables, size_t K, size_t n, Transcript& tr) {
  const size_t nv = lasso_batch_check(tables, K, n);
  argument_pcs_check(pcs, "lasso batch");
  argument_verdict("lasso batch", [&] { lasso_verify_batch_checked(pcs, tables, K, n, nv, tr); });
}

// ------------------------------------------------------------------ Brakedown (pcs/multilinear/brakedown.rs:315-396)
void brakedown_verify(const BdParam& p, const uint8_t root[32], const HFr* point, size_t num_vars, const HFr& eval,
                      Transcript& tr, HashTranscript& ht) {
  if (num_vars != p.num_vars)
    throw Error(LH_ERR_INVALID_PCS_PARAM, "Invalid poly or point to verify (param supports " +
                                              std::to_string(p.num_vars) + " variates but got " +
                                              std::to_string(num_vars) + ")");
  const size_t R = p.num_rows, row_len = p.row_len, cw = p.codeword_len;
  size_t k_rows = 0;
  while (((size_t)1 << k_rows) < R) k_rows++;
  const std::vector<HFr> t_0 = host_eq_xy(std::vector<HFr>(point + num_vars - k_rows, point + num_vars));
  const std::vector<HFr> t_1 = host_eq_xy(std::vector<HFr>(point, point + num_vars - k_rows));
  std::vector<std::pair<std::vector<HFr>, std::vector<HFr>>> combined;  // (coefficients, encoded row)
  auto read_row = [&](std::vector<HFr> coeffs) {
    std::vector<HFr> row = tr.read_field_elements(row_len);
    row.resize(cw);
    brakedown_encode_host(p, row.data());
    combined.emplace_back(std::move(coeffs), std::move(row));
  };
  if (R > 1) read_row(tr.squeeze_challenges(R));
  read_row(t_0);
  for (size_t i = 0; i < p.num_column_opening; i++) {
    uint8_t repr[32];
    tr.squeeze_challenge().to_repr(repr);
    const size_t column = (size_t)(((uint32_t)repr[0] | (uint32_t)repr[1] << 8 | (uint32_t)repr[2] << 16 |
                                    (uint32_t)repr[3] << 24) % cw);
    const std::vector<HFr> items = tr.read_field_elements(R);
    std::vector<uint8_t> path(32 * p.depth);
    for (size_t k = 0; k < p.depth; k++) ht.read_hash(path.data() + 32 * k);
    for (const auto& cr : combined) {  // proximity
      HFr item = items[0];
      if (R > 1) {
        item = HFr::zero();
        for (size_t r = 0; r < R; r++) item += cr.first[r] * items[r];
      }
      if (item != cr.second[column]) throw Error(LH_ERR_INVALID_PCS_OPEN, "Proximity failure");
    }
    Keccak256 hasher;  // merkle tree opening
    uint8_t out[32], buf[64];
    for (const HFr& x : items) {
      x.to_repr(repr);
      hasher.update(repr, 32);
    }
    hasher.finalize_reset(out);
    for (size_t k = 0; k < p.depth; k++) {
      const bool left = ((column >> k) & 1) == 0;
      memcpy(buf + (left ? 0 : 32), out, 32);
      memcpy(buf + (left ? 32 : 0), path.data() + 32 * k, 32);
      hasher.update(buf, 64);
      hasher.finalize_reset(out);
    }
    if (memcmp(out, root, 32) != 0) throw Error(LH_ERR_INVALID_PCS_OPEN, "Invalid merkle tree opening");
  }
  HFr acc = HFr::zero();  // consistency
  for (size_t c = 0; c < row_len; c++) acc += combined.back().second[c] * t_1[c];
  if (acc != eval) throw Error(LH_ERR_INVALID_PCS_OPEN, "Consistency failure");
}

// ------------------------------------------------------------------ Lasso and HyperPlonk::verify over Brakedown
// A root travels through lasso_verify / hyperplonk_verify_phases in the first 32 bytes of a 64-byte commitment slot; instance
// polys keep the all-zero slot and are never queried (verifier.rs:147-154).
static PcsVerifier brakedown_verifier(const BdParam& p, HashTranscript& ht) {
  PcsVerifier pcs;
  pcs.batch_verify = [&p, &ht](size_t nv, const HG1* comms, size_t nc, const HFr* points, size_t np, const lh_evaluation* evals,
                               size_t ne, Transcript& t2) {
    for (size_t i = 0; i < ne; i++) {  // batch_verify is one verify per evaluation (brakedown.rs:398-417)
      const lh_evaluation& e = evals[i];
      LH_REQUIRE(e.poly < nc && e.point < np, LH_ERR_ARG, "brakedown batch_verify: evaluation out of range");
      HFr v;
      memcpy(&v, &e.value, 32);
      brakedown_verify(p, (const uint8_t*)&comms[e.poly], points + (size_t)e.point * nv, nv, v, t2, ht);
    }
  };
  pcs.read_commitments = [&ht](Transcript&, size_t n) {
    std::vector<HG1> v(n);
    if (n) memset((void*)v.data(), 0, n * sizeof(HG1));
    for (size_t i = 0; i < n; i++) ht.read_hash((uint8_t*)&v[i]);
    return v;
  };
  return pcs;
}

void brakedown_lasso_verify(const BdParam& p, const lh_lasso_table& tb, size_t n, Transcript& tr, HashTranscript& ht) {
  lasso_verify_check_table(tb, n);
  if (std::max<size_t>(n, tb.chunk_bits) != p.num_vars)  // (brakedown_verify's own refusal, ahead of the argument)
    throw Error(LH_ERR_INVALID_PCS_PARAM, "Invalid poly or point to verify (param supports " + std::to_string(p.num_vars) +
                                              " variates but got " + std::to_string(std::max<size_t>(n, tb.chunk_bits)) + ")");
  lasso_verify(brakedown_verifier(p, ht), tb, n, tr);
}

void brakedown_hyperplonk_verify_phases(const BdParam& p, const lh_hp_vparam& vp, const uint8_t* preprocess_roots,
                                        const uint8_t* permutation_roots, const std::vector<size_t>& num_witness_polys,
                                        const std::vector<size_t>& num_challenges, const HFr* const* instances,
                                        Transcript& tr, HashTranscript& ht) {
  LH_REQUIRE(vp.num_lasso_lookups == 0, LH_ERR_ARG,
             "hyperplonk over brakedown: Lasso lookups are not supported (their column commitments are points)");
  LH_REQUIRE(vp.num_vars == p.num_vars, LH_ERR_ARG,
             "hyperplonk over brakedown: the circuit has " + std::to_string(vp.num_vars) + " variables, the param " +
                 std::to_string(p.num_vars));
  auto slots = [](const uint8_t* roots, size_t n) {
    std::vector<lh_g1> v(std::max<size_t>(n, 1));
    memset(v.data(), 0, v.size() * sizeof(lh_g1));
    for (size_t i = 0; i < n; i++) memcpy(&v[i], roots + 32 * i, 32);
    return v;
  };
  const std::vector<lh_g1> pre = slots(preprocess_roots, vp.num_preprocess_polys),
                           perm = slots(permutation_roots, vp.num_permutation_polys);
  lh_hp_vparam v2 = vp;
  v2.preprocess_comms = pre.data(), v2.permutation_comms = perm.data();
  const PcsVerifier pcs = brakedown_verifier(p, ht);
  hyperplonk_verify_phases(pcs, v2, num_witness_polys, num_challenges, instances, tr);
}

}  // namespace lh
