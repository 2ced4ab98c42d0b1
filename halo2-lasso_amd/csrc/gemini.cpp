// Gemini over univariate KZG, and the batched univariate KZG opening under it: prover half (reference
// pcs/multilinear/gemini.rs:56-155, pcs/univariate/kzg.rs:242-354,422-555).  A Gemini opening of an n-variable table
// (committed as a coefficient vector against the powers of s, the same bytes as Zeromorph's commitment) is
//   n - 1 fold commitments           one msm_batch over the flat fold buffer
//   n evaluations                    fs[0](-beta), fs[i](-beta^(2^i)): one even/odd pass over every fold
//   UnivariateKzg::batch_open        [q], q = sum_S gamma^S (f_S div Z_S), then the single-point opening of
//                                    f = sum_S scalar_S f_S + q_scalar q at z
// A quotient by a set's vanishing polynomial is taken factor by factor (suffix Horner, remainders dropped: with
// f = q_1 (X - p_1) + r_1 and q_1 = q_2 (X - p_2) + r_2, q_2 is the quotient by the product); two points p, -p of a set go
// as ONE factor X^2 - p^2 (a stride-2 suffix Horner) - Gemini's first set is exactly that.  All sets of one opening share
// the launches of a factor round.  Restated in tests/gemini_ref.py (schoolbook division by the expanded vanishing
// polynomial), which the tests compare against byte for byte.
#include <algorithm>
#include "host.hpp"

namespace lh {

static void check_trim(const USrs& srs, size_t poly_size) {
  LH_REQUIRE(poly_size >= 1 && poly_size <= srs.size, LH_ERR_INVALID_PCS_PARAM, "Too large poly_size to trim to");
}
static void check_len(size_t poly_size, size_t len, const char* what) {  // pp.degree() < poly.degree() (kzg.rs:243,272)
  if (len > poly_size)
    throw Error(LH_ERR_INVALID_PCS_PARAM, std::string("Too large degree of poly to ") + what + " (param supports degree up to " +
                                              std::to_string(poly_size - 1) + " but got " + std::to_string(len - 1) + ")");
}
static void check_vars(const USrs& srs, size_t poly_size, size_t num_vars, const char* what) {  // gemini.rs:57,87
  check_trim(srs, poly_size);
  if (num_vars >= 63 || ((size_t)1 << num_vars) > poly_size)
    throw Error(LH_ERR_INVALID_PCS_PARAM, std::string("Too large degree of poly to ") + what + " (param supports degree up to " +
                                              std::to_string(poly_size - 1) + " but got " +
                                              (num_vars >= 63 ? std::string("2^") + std::to_string(num_vars) : std::to_string((size_t)1 << num_vars)) + ")");
}

// commit_coeffs (kzg.rs:24-31) of several coefficient vectors in one MSM batch; an empty vector commits to the identity
static std::vector<HG1> commit_coeffs(Ctx& c, const USrs& srs, const UPoly* polys, size_t num_polys) {
  std::vector<HG1> out(num_polys, HG1{host::Fq::zero(), host::Fq::zero()});
  std::vector<MsmJob> jobs;
  std::vector<size_t> idx;
  for (size_t i = 0; i < num_polys; i++)
    if (polys[i].len) {
      jobs.push_back(MsmJob{polys[i].d, false, srs.d_powers, polys[i].len});
      idx.push_back(i);
    }
  if (jobs.empty()) return out;
  std::vector<HG1> got(jobs.size());
  msm_batch(c, jobs.data(), jobs.size(), (G1Affine*)got.data());
  for (size_t k = 0; k < idx.size(); k++) out[idx[k]] = got[k];
  return out;
}

std::vector<HG1> ukzg_batch_commit(Ctx& c, const USrs& srs, size_t poly_size, const UPoly* polys, size_t num_polys) {
  check_trim(srs, poly_size);
  for (size_t i = 0; i < num_polys; i++) check_len(poly_size, polys[i].len, "commit");
  return commit_coeffs(c, srs, polys, num_polys);
}

// kzg.rs:264-299: the quotient of poly by X - point is out[1..] of the suffix Horner scan
void ukzg_open(Ctx& c, const USrs& srs, size_t poly_size, const UPoly& poly, const HFr& point, Transcript& tr) {
  check_trim(srs, poly_size);
  check_len(poly_size, poly.len, "open");
  ArenaScope scope(c.arena);
  UPoly quotient{nullptr, 0};
  if (poly.len > 1) {
    Fr* S = c.arena.alloc_n<Fr>(poly.len);
    GmHornerSeg seg{poly.d, S, poly.len, 1, dev(point)};
    k_gm_suffix_horner(c, &seg, 1);
    quotient = UPoly{S + 1, poly.len - 1};
  }
  tr.write_commitment(commit_coeffs(c, srs, &quotient, 1)[0]);
}

void ukzg_batch_open(Ctx& c, const USrs& srs, size_t poly_size, const UPoly* polys, size_t num_polys, const HFr* points,
                     size_t num_points, const lh_evaluation* evals, size_t num_evals, Transcript& tr) {
  check_trim(srs, poly_size);
  LH_REQUIRE(num_evals >= 1, LH_ERR_ARG, "univariate batch open: no evaluations");
  for (size_t i = 0; i < num_evals; i++)
    LH_REQUIRE(evals[i].poly < num_polys && evals[i].point < num_points, LH_ERR_ARG, "univariate batch open: bad evaluation");
  for (size_t i = 0; i < num_polys; i++) check_len(poly_size, polys[i].len, "open");
  const UkzgEvalSets es = ukzg_eval_sets(evals, num_evals);
  const std::vector<UkzgEvalSet>& sets = es.sets;
  const HFr beta = tr.squeeze_challenge(), gamma = tr.squeeze_challenge();
  size_t max_set_len = 0;
  for (auto& s : sets) max_set_len = std::max(max_set_len, s.polys.size());
  std::vector<HFr> pob(max_set_len), pog(sets.size());
  pob[0] = HFr::one();
  for (size_t i = 1; i < max_set_len; i++) pob[i] = pob[i - 1] * beta;
  pog[0] = HFr::one();
  for (size_t i = 1; i < sets.size(); i++) pog[i] = pog[i - 1] * gamma;

  ArenaScope scope(c.arena);
  // f_S = sum_k beta^k poly_k (a set of one poly is that poly itself)
  std::vector<UPoly> fs(sets.size());
  for (size_t s = 0; s < sets.size(); s++) {
    if (sets[s].polys.size() == 1) {
      fs[s] = polys[sets[s].polys[0]];
      continue;
    }
    std::vector<GmTerm> terms;
    size_t len = 0;
    for (size_t k = 0; k < sets[s].polys.size(); k++) {
      const UPoly& p = polys[sets[s].polys[k]];
      terms.push_back(GmTerm{p.d, p.len, dev(pob[k])});
      len = std::max(len, p.len);
    }
    Fr* f = c.arena.alloc_n<Fr>(std::max<size_t>(len, 1));
    k_gm_combine(c, terms.data(), terms.size(), len, f);
    fs[s] = UPoly{f, len};
  }
  // q = sum_S gamma^S (f_S div prod_{p in S} (X - p))
  size_t q_len = 0;
  for (size_t s = 0; s < sets.size(); s++) {
    const size_t deg = sets[s].points.size();
    if (fs[s].len > deg) q_len = std::max(q_len, fs[s].len - deg);
  }
  Fr* q = c.arena.alloc_n<Fr>(std::max<size_t>(q_len, 1));
  {
    ArenaScope div_scope(c.arena);
    struct Factor {
      uint32_t stride;
      HFr x;
    };
    std::vector<std::vector<Factor>> factors(sets.size());
    size_t rounds = 0;
    for (size_t s = 0; s < sets.size(); s++) {
      std::vector<HFr> pts;
      for (size_t i : sets[s].points) pts.push_back(points[i]);
      std::vector<char> used(pts.size(), 0);
      for (size_t a = 0; a < pts.size(); a++) {
        if (used[a]) continue;
        used[a] = 1;
        size_t b = a + 1;
        while (b < pts.size() && (used[b] || !(pts[a] + pts[b]).is_zero())) b++;
        if (b < pts.size()) {
          used[b] = 1;
          factors[s].push_back(Factor{2, pts[a].sqr()});
        } else {
          factors[s].push_back(Factor{1, pts[a]});
        }
      }
      rounds = std::max(rounds, factors[s].size());
    }
    std::vector<UPoly> cur = fs;
    for (size_t r = 0; r < rounds; r++) {
      std::vector<GmHornerSeg> segs;
      std::vector<size_t> owner;
      for (size_t s = 0; s < sets.size(); s++) {
        if (r >= factors[s].size() || !cur[s].len) continue;
        const Factor& fa = factors[s][r];
        if (cur[s].len <= fa.stride) {  // the dividend's degree is below the divisor's: the quotient is zero
          cur[s] = UPoly{nullptr, 0};
          continue;
        }
        Fr* out = c.arena.alloc_n<Fr>(cur[s].len);
        segs.push_back(GmHornerSeg{cur[s].d, out, cur[s].len, fa.stride, dev(fa.x)});
        owner.push_back(s);
      }
      k_gm_suffix_horner(c, segs.data(), segs.size());
      for (size_t k = 0; k < segs.size(); k++) cur[owner[k]] = UPoly{segs[k].out + segs[k].stride, segs[k].len - segs[k].stride};
    }
    std::vector<GmTerm> terms;
    for (size_t s = 0; s < sets.size(); s++)
      if (cur[s].len) terms.push_back(GmTerm{cur[s].d, cur[s].len, dev(pog[s])});
    k_gm_combine(c, terms.data(), terms.size(), q_len, q);
  }
  const UPoly q_poly{q, q_len};
  tr.write_commitment(commit_coeffs(c, srs, &q_poly, 1)[0]);

  const HFr z = tr.squeeze_challenge();
  auto sc = ukzg_set_scalars(sets, pog, points, z);
  const HFr q_scalar = -(ukzg_vanishing_eval(es.superset, points, z) * sc.second);
  // f = sum_S scalar_S f_S + q_scalar q, then UnivariateKzg::open at z (its comm and eval are not written)
  std::vector<GmTerm> terms;
  size_t f_len = q_len;
  for (size_t s = 0; s < sets.size(); s++) {
    terms.push_back(GmTerm{fs[s].d, fs[s].len, dev(sc.first[s])});
    f_len = std::max(f_len, fs[s].len);
  }
  terms.push_back(GmTerm{q, q_len, dev(q_scalar)});
  Fr* f = c.arena.alloc_n<Fr>(std::max<size_t>(f_len, 1));
  k_gm_combine(c, terms.data(), terms.size(), f_len, f);
  ukzg_open(c, srs, poly_size, UPoly{f, f_len}, z, tr);
}

// ------------------------------------------------------------------ Gemini
std::vector<HG1> gemini_batch_commit(Ctx& c, const USrs& srs, size_t poly_size, const Fr* const* d_polys, size_t num_polys,
                                     size_t num_vars) {
  check_vars(srs, poly_size, num_vars, "commit");
  std::vector<UPoly> polys(num_polys);
  for (size_t i = 0; i < num_polys; i++) polys[i] = UPoly{d_polys[i], (size_t)1 << num_vars};
  return commit_coeffs(c, srs, polys.data(), num_polys);
}

void gemini_folds(Ctx& c, const Fr* d_poly, size_t num_vars, const HFr* point, Fr* d_out) {
  LH_REQUIRE(num_vars >= 1 && num_vars <= (size_t)GM_MAX_VARS, LH_ERR_ARG, "gemini: bad num_vars");
  std::vector<Fr> xs(num_vars);
  for (size_t i = 0; i + 1 < num_vars; i++) xs[i] = dev(point[i]);
  k_gm_fold_chain(c, d_poly, num_vars, xs.data(), d_out);
}

void gemini_open(Ctx& c, const USrs& srs, size_t poly_size, const Fr* d_poly, size_t num_vars, const HFr* point,
                 Transcript& tr) {
  check_vars(srs, poly_size, num_vars, "open");
  LH_REQUIRE(num_vars >= 1 && num_vars < (size_t)GM_MAX_VARS, LH_ERR_ARG, "gemini open: bad num_vars");
  const size_t n = (size_t)1 << num_vars;
  ArenaScope scope(c.arena);
  // fs[0] = poly, fs[i] at folds + off_i (gemini.rs:100-108)
  Fr* folds = c.arena.alloc_n<Fr>(std::max<size_t>(n - 2, 1));
  gemini_folds(c, d_poly, num_vars, point, folds);
  std::vector<UPoly> fs(num_vars);
  fs[0] = UPoly{d_poly, n};
  for (size_t i = 1, off = 0; i < num_vars; i++) {
    fs[i] = UPoly{folds + off, n >> i};
    off += n >> i;
  }
  tr.write_commitments(commit_coeffs(c, srs, fs.data() + 1, num_vars - 1));

  const HFr beta = tr.squeeze_challenge();
  std::vector<HFr> sq(num_vars + 1);  // squares(beta)
  sq[0] = beta;
  for (size_t i = 0; i < num_vars; i++) sq[i + 1] = sq[i].sqr();
  std::vector<HFr> points(num_vars + 1);
  points[0] = beta;
  for (size_t i = 0; i < num_vars; i++) points[i + 1] = -sq[i];
  // fs[i](p) = E_i(p^2) + p O_i(p^2): one pass over every fs[i], and fs[0](beta), fs[0](-beta) from the same pass
  std::vector<GmEvalSeg> segs(num_vars);
  for (size_t i = 0; i < num_vars; i++) segs[i] = GmEvalSeg{fs[i].d, fs[i].len, dev(sq[i + 1])};
  std::vector<Fr> eo(2 * num_vars);
  k_gm_eval_even_odd(c, segs.data(), num_vars, eo.data());
  std::vector<lh_evaluation> evals(num_vars + 1);
  auto set_eval = [&](size_t k, size_t poly, size_t pt, const HFr& v) {
    evals[k].poly = (uint32_t)poly, evals[k].point = (uint32_t)pt;
    memcpy(&evals[k].value, &v, 32);
  };
  set_eval(0, 0, 0, hst(eo[0]) + beta * hst(eo[1]));
  std::vector<HFr> written(num_vars);
  for (size_t i = 0; i < num_vars; i++) {
    written[i] = hst(eo[2 * i]) + points[i + 1] * hst(eo[2 * i + 1]);
    set_eval(i + 1, i, i + 1, written[i]);
  }
  tr.write_field_elements(written);
  ukzg_batch_open(c, srs, poly_size, fs.data(), num_vars, points.data(), num_vars + 1, evals.data(), num_vars + 1, tr);
}

void gemini_batch_open(Ctx& c, const USrs& srs, size_t poly_size, size_t num_vars, const Fr* const* d_polys, size_t num_polys,
                       const HFr* points, size_t num_points, const lh_evaluation* evals, size_t num_evals, Transcript& tr,
                       const SmallPoly* small) {
  check_vars(srs, poly_size, num_vars, "open");
  additive_batch_open(
      c, num_vars, d_polys, num_polys, points, num_points, evals, num_evals, tr,
      [&](const Fr* g_prime, const HFr* point) { gemini_open(c, srs, poly_size, g_prime, num_vars, point, tr); }, small);
}

Pcs gemini_pcs(Ctx& c, const USrs& srs, size_t poly_size) {
  check_trim(srs, poly_size);
  Pcs p;
  p.batch_commit = [&c, &srs, poly_size](const Fr* const* polys, size_t np, size_t nv) {
    return gemini_batch_commit(c, srs, poly_size, polys, np, nv);
  };
  p.commit_bases = [&srs](size_t) { return (const G1Affine*)srs.d_powers; };
  while (((size_t)2 << p.max_vars) <= poly_size) p.max_vars++;
  p.batch_open = [&c, &srs, poly_size](size_t nv, const Fr* const* polys, size_t np, const HFr* points, size_t npts,
                                       const lh_evaluation* evals, size_t ne, Transcript& tr, const SmallPoly* small) {
    gemini_batch_open(c, srs, poly_size, nv, polys, np, points, npts, evals, ne, tr, small);
  };
  return p;
}

}  // namespace lh
