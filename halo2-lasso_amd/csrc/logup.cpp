// LogUp-GKR: a stand-alone lookup argument for unstructured tables looked up by value.  The LogUp identity
//   sum_i 1 / (gamma + f[i]) = sum_r m[r] / (gamma + t[r])
// is proved by two fractional sum-checks (gkr.cpp prove_fractional_sum_check; piop/gkr/fractional_sum_check.rs and the paper
// it cites) instead of a committed helper column: only the inputs and the small-valued multiplicities are committed.
// The reference holds no such argument; protocol and transcript schedule are specified in tests/logup_gkr_ref.py and
// reproduced here byte for byte.  Written against the PCS description (host.hpp Pcs / PcsVerifier), as lasso_prove_batch is.
#include <algorithm>
#include "host.hpp"

namespace lh {

size_t logup_check(const lh_logup_lookup* lookups, size_t L, size_t n, size_t l, bool prover) {
  LH_REQUIRE(lookups != nullptr, LH_ERR_ARG, "null argument: lookups");
  LH_REQUIRE(L >= 1 && L <= (size_t)LH_LOGUP_MAX_LOOKUPS, LH_ERR_ARG,
             "logup: 1 to " + std::to_string(LH_LOGUP_MAX_LOOKUPS) + " lookups");
  LH_REQUIRE(n >= 1 && n < 31, LH_ERR_ARG, "logup: num_vars out of range (1 to 30)");
  LH_REQUIRE(l >= 1 && l <= (size_t)LH_LOGUP_MAX_TABLE_VARS, LH_ERR_ARG,
             "logup: table_vars out of range (1 to " + std::to_string(LH_LOGUP_MAX_TABLE_VARS) + ")");
  size_t total = 0;
  for (size_t k = 0; k < L; k++) {
    const lh_logup_lookup& lk = lookups[k];
    LH_REQUIRE(lk.width >= 1 && lk.width <= (uint32_t)LH_LOGUP_MAX_WIDTH, LH_ERR_ARG,
               "logup: lookup " + std::to_string(k) + ": width out of range (1 to " + std::to_string(LH_LOGUP_MAX_WIDTH) + ")");
    LH_REQUIRE(lk.table != nullptr, LH_ERR_ARG, "null argument: table of lookup " + std::to_string(k));
    LH_REQUIRE(!prover || lk.d_inputs != nullptr, LH_ERR_ARG, "null argument: d_inputs of lookup " + std::to_string(k));
    for (uint32_t j = 0; j < lk.width; j++) {
      LH_REQUIRE(lk.table[j] != nullptr, LH_ERR_ARG, "null argument: a table column of lookup " + std::to_string(k));
      LH_REQUIRE(!prover || lk.d_inputs[j] != nullptr, LH_ERR_ARG, "null argument: an input column of lookup " + std::to_string(k));
    }
    total += lk.width;
  }
  // one identity mask (a field element read as 63 bits) frames the input commitments
  LH_REQUIRE(total <= 63, LH_ERR_ARG, "logup: more than 63 input columns in all (one identity mask)");
  return std::max(n, l);
}

template <class Lookup>  // (lh_logup_lookup or lh_logup_columns: the widths)
static void logup_header(Transcript& tr, const Lookup* lookups, size_t L, size_t n, size_t l) {
  for (size_t v : {L, n, l}) tr.common_field_element(HFr::from_u64(v));
  for (size_t k = 0; k < L; k++) tr.common_field_element(HFr::from_u64(lookups[k].width));
}
// beta^0 .. beta^(LH_LOGUP_MAX_WIDTH - 1)
static std::vector<HFr> logup_powers(const HFr& beta) {
  std::vector<HFr> pw(LH_LOGUP_MAX_WIDTH, HFr::one());
  for (size_t j = 1; j < pw.size(); j++) pw[j] = pw[j - 1] * beta;
  return pw;
}
// the opening list shared by prover and verifier: input column i at point 0 (x_n), m_k (poly W + k) at point 1 (x_l)
static std::vector<lh_evaluation> logup_evaluations(const std::vector<HFr>& f_e, const std::vector<HFr>& m_e) {
  std::vector<lh_evaluation> evs;
  for (const HFr& v : f_e) evs.push_back(make_evaluation(evs.size(), 0, &v));
  for (const HFr& v : m_e) evs.push_back(make_evaluation(evs.size(), 1, &v));
  return evs;
}

// the limits of the prover over columns of either kind: those of logup_check on the same lists, then the kinds
static size_t logup_columns_check(const lh_logup_columns* lookups, size_t L, size_t n, size_t l) {
  LH_REQUIRE(lookups != nullptr, LH_ERR_ARG, "null argument: lookups");
  std::vector<lh_logup_lookup> plain(LH_LOGUP_MAX_LOOKUPS);  // (a count out of range is logup_check's to refuse)
  for (size_t k = 0; k < std::min<size_t>(L, plain.size()); k++)
    plain[k] = lh_logup_lookup{lookups[k].width, (const lh_fr* const*)lookups[k].d_inputs, lookups[k].table};
  const size_t nv = logup_check(plain.data(), L, n, l, true);
  for (size_t k = 0; k < L; k++)
    for (uint32_t j = 0; lookups[k].kinds && j < lookups[k].width; j++)
      LH_REQUIRE(lookups[k].kinds[j] == LH_LOGUP_COL_FR || lookups[k].kinds[j] == LH_LOGUP_COL_U32, LH_ERR_ARG,
                 "logup: lookup " + std::to_string(k) + ", column " + std::to_string(j) + ": unknown column kind " +
                     std::to_string(lookups[k].kinds[j]));
  return nv;
}

void logup_gkr_prove(Ctx& c, const Pcs& pcs, const lh_logup_lookup* lookups, size_t L, size_t n, size_t l, Transcript& tr) {
  logup_check(lookups, L, n, l, true);
  std::vector<lh_logup_columns> cols(L);
  for (size_t k = 0; k < L; k++)
    cols[k] = lh_logup_columns{lookups[k].width, (const void* const*)lookups[k].d_inputs, nullptr, lookups[k].table};
  logup_gkr_prove_columns(c, pcs, cols.data(), L, n, l, tr);
}

// One body for both entries; the kind is a property of a column.  A u32 column is committed, compressed, evaluated and opened
// as the 32-bit column it is (never widened, never padded) - the way the multiplicities go.
void logup_gkr_prove_columns(Ctx& c, const Pcs& pcs, const lh_logup_columns* lookups, size_t L, size_t n, size_t l,
                             Transcript& tr) {
  const size_t nv = logup_columns_check(lookups, L, n, l);
  argument_not_sharded(c, "logup");
  argument_pcs_check(pcs, nv, "logup", true);
  const size_t N = (size_t)1 << n, M = (size_t)1 << l, NV = (size_t)1 << nv;
  open_precommit_cancel(c);
  ArenaScope scope(c.arena);
  EqHalfScope eq_scope(c);  // (the opening shares eq tables of its points: arena memory of this scope)
  size_t W = 0;
  std::vector<size_t> first(L);  // the first input column of every lookup
  for (size_t k = 0; k < L; k++) first[k] = W, W += lookups[k].width;

  // ---- 0/1: header, the input columns' commitments, lookup-major in column order whatever the kinds.  An Fr column is
  // zero-padded to nv variables (the table the opening is handed too); a u32 column is a 32-bit MSM over its 2^n entries
  // against the bases of level nv, its width promised from the OR of its entries - neither widened nor padded
  logup_header(tr, lookups, L, n, l);
  std::vector<const void*> f(W);              // input column i as it was handed in ...
  std::vector<uint8_t> u32(W, 0);             // ... a uint32_t column?
  std::vector<size_t> fr_at, sm_at;           // the columns of either kind, in column order
  std::vector<const Fr*> polys(W + L, nullptr);  // the opening's tables (null: a 32-bit column, SmallPoly below)
  std::vector<uint32_t> f_bits(W, 0);
  for (size_t k = 0; k < L; k++)
    for (uint32_t j = 0; j < lookups[k].width; j++) {
      const size_t i = first[k] + j;
      f[i] = lookups[k].d_inputs[j];
      u32[i] = lookups[k].kinds != nullptr && lookups[k].kinds[j] == LH_LOGUP_COL_U32;
      (u32[i] ? sm_at : fr_at).push_back(i);
      if (u32[i]) continue;
      const Fr* col = (const Fr*)f[i];
      polys[i] = col;
      if (N < NV) {
        Fr* pad = c.arena.alloc_n<Fr>(NV);
        LH_HIP(hipMemcpyAsync(pad, col, N * sizeof(Fr), hipMemcpyDeviceToDevice, c.stream));
        LH_HIP(hipMemsetAsync(pad + N, 0, (NV - N) * sizeof(Fr), c.stream));
        polys[i] = pad;
      }
    }
  {
    std::vector<HG1> comms(W);
    if (!fr_at.empty()) {
      std::vector<const Fr*> tables;
      for (size_t i : fr_at) tables.push_back(polys[i]);
      const std::vector<HG1> out = pcs.batch_commit(tables.data(), tables.size(), nv);
      for (size_t t = 0; t < fr_at.size(); t++) comms[fr_at[t]] = out[t];
    }
    if (!sm_at.empty()) {
      std::vector<U32Column> cols;
      for (size_t i : sm_at) cols.push_back(U32Column{(const uint32_t*)f[i], N});
      std::vector<uint32_t> bits(cols.size());
      const std::vector<HG1> out = commit_u32_columns(c, pcs, nv, cols, bits.data());
      for (size_t t = 0; t < sm_at.size(); t++) comms[sm_at[t]] = out[t], f_bits[sm_at[t]] = bits[t];
    }
    lasso_write_commitments(tr, comms);
  }

  // ---- 2: beta, the compressed columns cf_k (device inputs) and ct_k (the public table, uploaded)
  const std::vector<HFr> pw = logup_powers(tr.squeeze_challenge());
  std::vector<const Fr*> cf(L), ct(L);
  for (size_t k = 0; k < L; k++) {
    const size_t w = lookups[k].width;
    std::vector<const Fr*> t(w);
    for (size_t j = 0; j < w; j++) {
      Fr* d = c.arena.alloc_n<Fr>(M);
      LH_HIP(hipMemcpyAsync(d, lookups[k].table[j], M * sizeof(Fr), hipMemcpyHostToDevice, c.stream));
      t[j] = d;
    }
    cf[k] = (const Fr*)f[first[k]], ct[k] = t[0];  // (w = 1 and an Fr column: the column itself, nothing launched)
    const bool any_u32 = std::any_of(u32.begin() + first[k], u32.begin() + first[k] + w, [](uint8_t b) { return b != 0; });
    if (any_u32) {  // (the join and the leaves read cf_k as field elements: a single u32 column is widened by the same kernel)
      Fr* dcf = c.arena.alloc_n<Fr>(N);
      k_logup_compress_cols(c, f.data() + first[k], u32.data() + first[k], (const Fr*)pw.data(), w, N, dcf);
      cf[k] = dcf;
    } else if (w > 1) {
      Fr* dcf = c.arena.alloc_n<Fr>(N);
      k_logup_compress(c, (const Fr* const*)(f.data() + first[k]), (const Fr*)pw.data(), w, N, dcf);
      cf[k] = dcf;
    }
    if (w > 1) {
      Fr* dct = c.arena.alloc_n<Fr>(M);
      k_logup_compress(c, t.data(), (const Fr*)pw.data(), w, M, dct);
      ct[k] = dct;
    }
  }

  // ---- 3: multiplicities (prover.rs:145-192 lookup_m_poly: the LAST of equal rows takes every count) as u32 columns, committed
  // like the u32 inputs (commit_u32_columns)
  std::vector<uint32_t*> m(L);
  std::vector<uint32_t> m_bits(L);
  {
    std::vector<U32Column> cols;
    for (size_t k = 0; k < L; k++) {
      m[k] = c.arena.alloc_n<uint32_t>(M + 1);
      if (!k_logup_multiplicities(c, cf[k], N, ct[k], M, m[k])) throw Error(LH_ERR_INVALID_SNARK, "Invalid lookup input");
      cols.push_back(U32Column{m[k], M});
    }
    lasso_write_commitments(tr, commit_u32_columns(c, pcs, nv, cols, m_bits.data()));
  }

  // ---- 4-6: gamma, the leaves of both sides (and, fused, the level above them), the two fractional sum-checks
  const HFr gamma = tr.squeeze_challenge();
  const bool fused = c.opt.logup_fused_leaves != 0;
  auto side = [&](bool table_side, size_t vars, const std::vector<const Fr*>& cols) {
    const size_t len = (size_t)1 << vars;
    const bool up = fused && vars >= 2;  // (one variable: the leaves are the top layer)
    LogupLeaves a;
    memset(&a, 0, sizeof(a));
    std::vector<const Fr*> ps(L), qs(L), p_up(L), q_up(L);
    if (!table_side) a.ones = c.arena.alloc_n<Fr>(len);
    for (size_t k = 0; k < L; k++) {
      a.c[k] = cols[k];
      a.q[k] = c.arena.alloc_n<Fr>(len);
      if (table_side) a.m[k] = m[k], a.p[k] = c.arena.alloc_n<Fr>(len);
      if (up) a.p_up[k] = c.arena.alloc_n<Fr>(len / 2), a.q_up[k] = c.arena.alloc_n<Fr>(len / 2);
      ps[k] = table_side ? a.p[k] : a.ones, qs[k] = a.q[k], p_up[k] = a.p_up[k], q_up[k] = a.q_up[k];
    }
    k_logup_leaves(c, a, L, vars, table_side, up, dev(gamma));
    return prove_fractional_sum_check(c, L, vars, nullptr, nullptr, ps.data(), qs.data(), tr, up ? p_up.data() : nullptr,
                                      up ? q_up.data() : nullptr);
  };
  const std::vector<HFr> x_n = side(false, n, cf).x;
  const std::vector<HFr> x_l = side(true, l, ct).x;

  // ---- 7: f_kj(x_n) lookup-major, then m_k(x_l)
  std::vector<HFr> f_e(W);
  if (!fr_at.empty()) {
    std::vector<const Fr*> tables;
    for (size_t i : fr_at) tables.push_back((const Fr*)f[i]);
    const std::vector<HFr> out = evaluate_polys(c, tables.data(), tables.size(), n, x_n.data());
    for (size_t t = 0; t < fr_at.size(); t++) f_e[fr_at[t]] = out[t];
  }
  if (!sm_at.empty()) {  // the u32 columns against eq(x_n), as the multiplicities against eq(x_l) below
    std::vector<const uint32_t*> cols;
    for (size_t i : sm_at) cols.push_back((const uint32_t*)f[i]);
    std::vector<HFr> out(cols.size());
    evaluate_u32_columns(c, cols.data(), cols.size(), x_n.data(), n, out.data());
    for (size_t t = 0; t < sm_at.size(); t++) f_e[sm_at[t]] = out[t];
  }
  std::vector<HFr> m_e(L);
  evaluate_u32_columns(c, m.data(), L, x_l.data(), l, m_e.data());
  tr.write_field_elements(f_e);
  tr.write_field_elements(m_e);

  // ---- 8: ONE batch opening over nv variables; the multiplicities and the u32 inputs go as their 32-bit columns.  When every
  // input is one, every opened poly is a small column and the opening takes them as columns (mkzg.cpp all_small; from
  // Options::open_small_min_vars on its largest quotients are committed column by column).  Nothing is committed ahead - no
  // Pcs::precommit call, the opening builds its column plan itself; the bytes do not depend on the route
  std::vector<SmallPoly> small(W + L);
  for (size_t i : sm_at) small[i] = SmallPoly{(const uint32_t*)f[i], N, f_bits[i]};
  for (size_t k = 0; k < L; k++) small[W + k] = SmallPoly{m[k], M, m_bits[k]};
  std::vector<HFr> points;
  lasso_append_points(points, {&x_n, &x_l}, nv);
  const std::vector<lh_evaluation> evs = logup_evaluations(f_e, m_e);
  pcs.batch_open(nv, polys.data(), polys.size(), points.data(), 2, evs.data(), evs.size(), tr, small.data());
}

// sum_j beta^j t~_j(x): the multilinear extension of the compressed table column, one fold over its 2^l rows; a row reads
// the w columns
static HFr logup_table_eval(const lh_logup_lookup& lk, size_t l, const std::vector<HFr>& pw, const std::vector<HFr>& x) {
  return host_table_eval(l, x, [&](size_t r) {
    HFr acc = ((const HFr*)lk.table[0])[r];
    for (uint32_t j = 1; j < lk.width; j++) acc += pw[j] * ((const HFr*)lk.table[j])[r];
    return acc;
  });
}

static void logup_gkr_verify_checked(const PcsVerifier& pcs, const lh_logup_lookup* lookups, size_t L, size_t n, size_t l, size_t nv,
                                     Transcript& tr) {
  size_t W = 0;
  for (size_t k = 0; k < L; k++) W += lookups[k].width;
  logup_header(tr, lookups, L, n, l);
  std::vector<HG1> comms = lasso_read_commitments(tr, W);
  const std::vector<HFr> pw = logup_powers(tr.squeeze_challenge());
  {
    const std::vector<HG1> block = lasso_read_commitments(tr, L);
    comms.insert(comms.end(), block.begin(), block.end());
  }
  const HFr gamma = tr.squeeze_challenge();
  const FracVerifyResult in = verify_fractional_sum_check(L, n, nullptr, nullptr, tr);
  const FracVerifyResult tb = verify_fractional_sum_check(L, l, nullptr, nullptr, tr);
  for (size_t k = 0; k < L; k++)  // the LogUp identity on the roots: P_f / Q_f + P_t / Q_t = 0
    if (!logup_roots_cancel(in.p_0s[k], in.q_0s[k], tb.p_0s[k], tb.q_0s[k]))
      throw Error(LH_ERR_INVALID_SNARK, "lookup " + std::to_string(k) + ": the fractions do not sum to zero");
  const std::vector<HFr> f_e = tr.read_field_elements(W), m_e = tr.read_field_elements(L);
  size_t at = 0;
  for (size_t k = 0; k < L; k++) {
    HFr q_in = gamma;
    for (uint32_t j = 0; j < lookups[k].width; j++) q_in += pw[j] * f_e[at + j];
    at += lookups[k].width;
    const HFr q_tab = gamma + logup_table_eval(lookups[k], l, pw, tb.x);
    if (in.p_xs[k] != HFr::one() || in.q_xs[k] != q_in || tb.p_xs[k] != HFr::zero() - m_e[k] || tb.q_xs[k] != q_tab)
      throw Error(LH_ERR_INVALID_SNARK, "lookup " + std::to_string(k) + ": leaf claim mismatch");
  }
  std::vector<HFr> points;
  lasso_append_points(points, {&in.x, &tb.x}, nv);
  const std::vector<lh_evaluation> evs = logup_evaluations(f_e, m_e);
  pcs.batch_verify(nv, comms.data(), comms.size(), points.data(), 2, evs.data(), evs.size(), tr);
}
void logup_gkr_verify(const PcsVerifier& pcs, const lh_logup_lookup* lookups, size_t L, size_t n, size_t l, Transcript& tr) {
  const size_t nv = logup_check(lookups, L, n, l, false);
  argument_pcs_check(pcs, "logup");
  argument_verdict("logup", [&] { logup_gkr_verify_checked(pcs, lookups, L, n, l, nv, tr); });
}

}  // namespace lh
