// Spark (Lasso paper section 4; the sparse commitment of Spartan): a sparse multilinear polynomial D in c l variables, given
// by 2^n entries (dim_0 .. dim_{c-1}, val), is committed ONCE at a cost that follows 2^n + 2^l, and its evaluations
//   D~(r_0 .. r_{c-1}) = sum_k val[k] prod_j eq(r_j, dim_j[k])
// are proved at any number of points: the memories E_j[k] = eq(r_j, dim_j[k]) are committed per opening, one sum-check over
// val prod_j E_j proves the value, and offline memory checking (one grand-product GKR, Init WS = RS Final) proves that every
// E_j was read from the eq table of r_j - whose extension the verifier knows in closed form.  The reference holds no such
// argument; protocol and transcript schedule are specified in tests/spark_ref.py and reproduced here byte for byte.
// Written against the PCS description (host.hpp Pcs / PcsVerifier), as logup.cpp is.
#include <algorithm>
#include "host.hpp"

namespace lh {

namespace {
// positions in an opening: [val | dim_j | read_ts_j | final_cts_j] (commitment order), then E_j; points 0 = r_z, 1 = r_N, 2 = r_M
struct SparkLayout {
  size_t c;
  size_t val() const { return 0; }
  size_t dim(size_t j) const { return 1 + j; }
  size_t read_ts(size_t j) const { return 1 + c + j; }
  size_t final_cts(size_t j) const { return 1 + 2 * c + j; }
  size_t E(size_t j) const { return 1 + 3 * c + j; }
  size_t committed() const { return 1 + 3 * c; }
  size_t num_polys() const { return 1 + 4 * c; }
};
// THE opening list: (val, r_z), (E_j, r_z).., (dim_j, r_N).., (read_ts_j, r_N).., (E_j, r_N).., (final_cts_j, r_M)..
// at_rz: val, E_0 ..; at_leaves: dim_j | read_ts_j | E_j at r_N, then final_cts_j at r_M - the order they are written in
std::vector<lh_evaluation> spark_evaluations(const SparkLayout& lay, const std::vector<HFr>& at_rz, const std::vector<HFr>& at_leaves) {
  const size_t c = lay.c;
  std::vector<lh_evaluation> evs;
  auto put = [&](size_t poly, size_t point, const HFr& v) { evs.push_back(make_evaluation(poly, point, &v)); };
  put(lay.val(), 0, at_rz[0]);
  for (size_t j = 0; j < c; j++) put(lay.E(j), 0, at_rz[1 + j]);
  for (size_t j = 0; j < c; j++) put(lay.dim(j), 1, at_leaves[j]);
  for (size_t j = 0; j < c; j++) put(lay.read_ts(j), 1, at_leaves[c + j]);
  for (size_t j = 0; j < c; j++) put(lay.E(j), 1, at_leaves[2 * c + j]);
  for (size_t j = 0; j < c; j++) put(lay.final_cts(j), 2, at_leaves[3 * c + j]);
  return evs;
}
// step 0 of an opening: n, l, c; the commitment's mask and its non-identity points; the point
void spark_header(Transcript& tr, size_t n, size_t l, size_t c, const std::vector<HG1>& comms, const HFr* point) {
  for (size_t v : {n, l, c}) tr.common_field_element(HFr::from_u64(v));
  uint64_t mask = 0;
  for (size_t i = 0; i < comms.size(); i++)
    if (comms[i].is_identity()) mask |= (uint64_t)1 << i;
  tr.common_field_element(HFr::from_u64(mask));
  for (const HG1& cm : comms)
    if (!cm.is_identity()) tr.common_commitment(cm);
  for (size_t i = 0; i < c * l; i++) tr.common_field_element(point[i]);
}
// every index below 2^l?  The OR of a column decides it exactly: 2^l is a power of two
void spark_range_check(Ctx& c, const uint32_t* const* dims, size_t cc, size_t N, size_t l, uint32_t* ors) {
  k_or_u32(c, dims, cc, N, ors);
  for (size_t j = 0; j < cc; j++)
    LH_REQUIRE(((uint64_t)ors[j] >> l) == 0, LH_ERR_ARG, "spark: index out of range (>= 2^dim_vars) in dimension " + std::to_string(j));
}
// the eq tables of the point's c parts (arena memory of the caller's scope)
void spark_eq_tables(Ctx& c, const HFr* point, size_t l, size_t cc, const Fr** T) {
  for (size_t j = 0; j < cc; j++) {
    Fr* t = c.arena.alloc_n<Fr>((size_t)1 << l);
    k_eq_xy(c, (const Fr*)(point + j * l), l, t);
    T[j] = t;
  }
}
}  // namespace

size_t spark_check(size_t n, size_t l, size_t c) {
  LH_REQUIRE(c >= 1 && c <= (size_t)LH_SPARK_MAX_DIMS, LH_ERR_ARG,
             "spark: num_dims out of range (1 to " + std::to_string(LH_SPARK_MAX_DIMS) + ")");
  LH_REQUIRE(l >= 1 && l <= (size_t)LH_SPARK_MAX_DIM_VARS, LH_ERR_ARG,
             "spark: dim_vars out of range (1 to " + std::to_string(LH_SPARK_MAX_DIM_VARS) + ")");
  // (Lasso's bound: the access counters and their sort index entries by 32-bit words)
  LH_REQUIRE(n >= 1 && n < 31, LH_ERR_ARG, "spark: num_vars out of range (1 to 30)");
  return std::max(n, l);
}

void spark_free(Ctx& c, SparkPoly* p) {
  auto it = std::find(c.spark_polys.begin(), c.spark_polys.end(), p);
  if (it == c.spark_polys.end()) return;
  c.spark_polys.erase(it);
  (void)hipStreamSynchronize(c.stream);  // (an opening queued on the stream may still read the columns)
  delete p;
}
void spark_free_all(Ctx& c) {
  while (!c.spark_polys.empty()) spark_free(c, c.spark_polys.back());
}

SparkPoly* spark_commit(Ctx& c, const Pcs& pcs, size_t n, size_t l, size_t cc, const uint32_t* const* d_dims, const Fr* d_val) {
  const size_t nv = spark_check(n, l, cc);
  LH_REQUIRE(d_dims != nullptr, LH_ERR_ARG, "null argument: d_dims");
  for (size_t j = 0; j < cc; j++) LH_REQUIRE(d_dims[j] != nullptr, LH_ERR_ARG, "null argument: d_dims[" + std::to_string(j) + "]");
  LH_REQUIRE(d_val != nullptr, LH_ERR_ARG, "null argument: d_val");
  argument_not_sharded(c, "spark");
  argument_pcs_check(pcs, nv, "spark", true);
  const size_t N = (size_t)1 << n, M = (size_t)1 << l, NV = (size_t)1 << nv;
  open_precommit_cancel(c);
  ArenaScope scope(c.arena);
  uint32_t or_dim[SPARK_MAX_DIMS];
  spark_range_check(c, d_dims, cc, N, l, or_dim);

  // ---- the handle's block: val padded to nv variables, then per dimension dim, read_ts (N words each) and final_cts (M)
  std::unique_ptr<SparkPoly> owner(new SparkPoly());
  SparkPoly& p = *owner;
  p.ctx = &c, p.n = n, p.l = l, p.c = cc, p.nv = nv;
  const size_t bytes = NV * sizeof(Fr) + cc * (2 * N + M) * sizeof(uint32_t);
  p.block.alloc(bytes);
  Fr* val = p.block.as<Fr>();
  uint32_t* words = (uint32_t*)(val + NV);
  LH_HIP(hipMemcpyAsync(val, d_val, N * sizeof(Fr), hipMemcpyDeviceToDevice, c.stream));
  if (N < NV) LH_HIP(hipMemsetAsync(val + N, 0, (NV - N) * sizeof(Fr), c.stream));
  p.val = val;
  uint32_t *rts[SPARK_MAX_DIMS], *fcs[SPARK_MAX_DIMS];
  for (size_t j = 0; j < cc; j++) {
    uint32_t* dim = words + j * (2 * N + M);
    LH_HIP(hipMemcpyAsync(dim, d_dims[j], N * sizeof(uint32_t), hipMemcpyDeviceToDevice, c.stream));
    p.dim[j] = dim, p.rts[j] = rts[j] = dim + N, p.fcs[j] = fcs[j] = dim + 2 * N;
  }
  // (the copies are checked columns: what the caller does to its own afterwards does not reach the handle.  Between the
  // check above and the copy the caller's columns are the caller's to leave alone, as during any prove)
  k_lasso_counters(c, p.dim, cc, N, M, rts, fcs);

  // ---- the commitments: val through batch_commit, every u32 column as a 32-bit MSM over its own length (commit_u32_columns;
  // the dims' ORs are the range check's), in commitment order (SparkLayout)
  p.comms = pcs.batch_commit(&p.val, 1, nv);
  {
    std::vector<U32Column> cols;
    for (size_t j = 0; j < cc; j++) cols.push_back(U32Column{p.dim[j], N, &or_dim[j]});
    for (size_t j = 0; j < cc; j++) cols.push_back(U32Column{p.rts[j], N});
    for (size_t j = 0; j < cc; j++) cols.push_back(U32Column{p.fcs[j], M});
    std::vector<uint32_t> bits(cols.size());
    const std::vector<HG1> out = commit_u32_columns(c, pcs, nv, cols, bits.data());
    p.comms.insert(p.comms.end(), out.begin(), out.end());
    for (size_t j = 0; j < cc; j++) p.dim_bits[j] = bits[j], p.rts_bits[j] = bits[cc + j], p.fcs_bits[j] = bits[2 * cc + j];
  }
  {
    KeccakTranscript kt;
    Transcript tr(&kt.vt);
    lasso_write_commitments(tr, p.comms);
    p.blob = kt.stream;
  }
  c.sync();
  c.spark_polys.push_back(&p);
  return owner.release();
}

HFr spark_open(Ctx& c, const Pcs& pcs, const SparkPoly& p, const HFr* point, Transcript& tr) {
  LH_REQUIRE(point != nullptr, LH_ERR_ARG, "null argument: point");
  LH_REQUIRE(std::find(c.spark_polys.begin(), c.spark_polys.end(), &p) != c.spark_polys.end(), LH_ERR_ARG,
             "spark: the polynomial was not committed on this ctx (or has been freed)");
  const size_t n = p.n, l = p.l, cc = p.c, nv = p.nv;
  argument_not_sharded(c, "spark");
  argument_pcs_check(pcs, nv, "spark", true);
  const size_t N = (size_t)1 << n, M = (size_t)1 << l, NV = (size_t)1 << nv;
  const SparkLayout lay{cc};
  open_precommit_cancel(c);
  ArenaScope scope(c.arena);
  EqHalfScope eq_scope(c);  // (the opening shares eq tables of its points: arena memory of this scope)

  // ---- 0/1: header; the eq tables of the point; the memories with the value in one launch; ONE block of c commitments
  spark_header(tr, n, l, cc, p.comms, point);
  const Fr* T[SPARK_MAX_DIMS];
  spark_eq_tables(c, point, l, cc, T);
  Fr* E[SPARK_MAX_DIMS];
  HFr v;
  {
    SparkE a;
    memset(&a, 0, sizeof(a));
    a.val = p.val;
    for (size_t j = 0; j < cc; j++) {
      E[j] = c.arena.alloc_n<Fr>(NV);  // (zero-padded to nv variables: the table the commitment and the opening are handed)
      if (N < NV) LH_HIP(hipMemsetAsync(E[j] + N, 0, (NV - N) * sizeof(Fr), c.stream));
      a.dim[j] = p.dim[j], a.T[j] = T[j], a.E[j] = E[j];
    }
    k_spark_e(c, a, cc, N, l, (Fr*)&v);
  }
  lasso_write_commitments(tr, pcs.batch_commit(E, cc, nv));

  // ---- 2/3: v; the sum-check of val prod_j E_j over n variables (no eq factor), then val and E_j at r_z
  tr.write_field_element(v);
  std::vector<HFr> r_z, at_rz;
  {
    lh_sop sop;
    memset(&sop, 0, sizeof(sop));
    sop.num_terms = 1, sop.global_eq = -1;
    const HFr one = HFr::one();
    memcpy(&sop.coeff[0], &one, 32);
    sop.num_factors[0] = (uint8_t)(cc + 1);
    const Fr* polys[1 + SPARK_MAX_DIMS] = {p.val};
    for (size_t j = 0; j <= cc; j++) sop.factor[0][j] = (uint8_t)j;
    for (size_t j = 0; j < cc; j++) polys[1 + j] = E[j];
    ScOptions so;
    so.sum_is_exact = true;
    SumCheckResult sc = sum_check_prove(c, LH_SC_EVALUATIONS, n, sop, polys, cc + 1, nullptr, 0, v, tr, so);
    r_z = sc.challenges, at_rz = sc.evals;
  }
  tr.write_field_elements(at_rz);

  // ---- 4/5: gamma, tau; the leaves of the 4 c trees in one launch (and, fused, the level above the large ones); the grand
  // product.  WS_j = RS_j + 1 goes to the tree builder as plus_one; it is stored only where that builder reads it: when the
  // n-variable trees are not alone at their leaf layer (n <= l) or no level above comes with them (as lasso.cpp)
  const HFr gamma = tr.squeeze_challenge(), tau = tr.squeeze_challenge();
  std::vector<HFr> r_N, r_M;
  {
    ArenaScope inner(c.arena);
    const bool fused = c.opt.logup_fused_leaves != 0;
    const bool up_n = fused && n >= GP_LEVEL_UP_MIN_VARS, up_l = fused && l >= GP_LEVEL_UP_MIN_VARS;
    const bool ws_implicit = up_n && n > l;
    SparkLeaves a;
    memset(&a, 0, sizeof(a));
    MemoryTrees trees(cc, n);
    for (size_t j = 0; j < cc; j++) {
      const MemoryTrees::Memory m = trees.add(c, j, N, l, up_n, ws_implicit, up_l);
      a.dim[j] = p.dim[j], a.rts[j] = p.rts[j], a.fcs[j] = p.fcs[j], a.E[j] = E[j], a.T[j] = T[j];
      a.rs[j] = m.rs, a.ws[j] = m.ws, a.rs_up[j] = m.rs_up, a.ws_up[j] = m.ws_up;
      a.init[j] = m.init, a.fin[j] = m.fin, a.init_up[j] = m.init_up, a.fin_up[j] = m.fin_up;
    }
    k_spark_leaves(c, a, cc, N, l, up_n, up_l, dev(gamma), dev(gamma * gamma), dev(tau));
    const GrandProductResult gp = trees.prove(c, tr);
    r_N = gp.points[0], r_M = gp.points[2 * cc];
  }

  // ---- 6: dim_j | read_ts_j | E_j at r_N, final_cts_j at r_M: the u32 columns against the eq table of their point
  std::vector<HFr> at_leaves(4 * cc);
  {
    std::vector<const uint32_t*> cols(p.dim, p.dim + cc);
    cols.insert(cols.end(), p.rts, p.rts + cc);
    evaluate_u32_columns(c, cols.data(), cols.size(), r_N.data(), n, at_leaves.data());
  }
  {
    const std::vector<HFr> e = evaluate_polys(c, E, cc, n, r_N.data());
    std::copy(e.begin(), e.end(), at_leaves.begin() + 2 * cc);
  }
  evaluate_u32_columns(c, p.fcs, cc, r_M.data(), l, at_leaves.data() + 3 * cc);
  tr.write_field_elements(at_leaves);

  // ---- 7: ONE batch opening over nv variables: the u32 columns go as their 32-bit columns, val and E_j as tables - the mixed
  // route of Lasso's product tables.  Nothing is committed ahead; the bytes do not depend on the route
  std::vector<const Fr*> polys(lay.num_polys(), nullptr);
  std::vector<SmallPoly> small(lay.num_polys());
  polys[lay.val()] = p.val;
  for (size_t j = 0; j < cc; j++) {
    small[lay.dim(j)] = SmallPoly{p.dim[j], N, p.dim_bits[j]};
    small[lay.read_ts(j)] = SmallPoly{p.rts[j], N, p.rts_bits[j]};
    small[lay.final_cts(j)] = SmallPoly{p.fcs[j], M, p.fcs_bits[j]};
    polys[lay.E(j)] = E[j];
  }
  std::vector<HFr> points;
  lasso_append_points(points, {&r_z, &r_N, &r_M}, nv);
  const std::vector<lh_evaluation> evs = spark_evaluations(lay, at_rz, at_leaves);
  pcs.batch_open(nv, polys.data(), polys.size(), points.data(), 3, evs.data(), evs.size(), tr, small.data());
  return v;
}

HFr spark_debug_e(Ctx& c, size_t n, size_t l, size_t cc, const uint32_t* const* d_dims, const Fr* d_val, const HFr* point,
                  Fr* const* d_E) {
  spark_check(n, l, cc);
  LH_REQUIRE(d_dims && d_val && point && d_E, LH_ERR_ARG, "null argument: d_dims, d_val, point or d_E");
  for (size_t j = 0; j < cc; j++) LH_REQUIRE(d_dims[j] && d_E[j], LH_ERR_ARG, "null argument: a column of d_dims or d_E");
  ArenaScope scope(c.arena);
  uint32_t ors[SPARK_MAX_DIMS];
  spark_range_check(c, d_dims, cc, (size_t)1 << n, l, ors);
  const Fr* T[SPARK_MAX_DIMS];
  spark_eq_tables(c, point, l, cc, T);
  SparkE a;
  memset(&a, 0, sizeof(a));
  a.val = d_val;
  for (size_t j = 0; j < cc; j++) a.dim[j] = d_dims[j], a.T[j] = T[j], a.E[j] = d_E[j];
  HFr v;
  k_spark_e(c, a, cc, (size_t)1 << n, l, (Fr*)&v);
  c.sync();
  return v;
}

static void spark_verify_checked(const PcsVerifier& pcs, size_t n, size_t l, size_t cc, size_t nv, const uint8_t* commitment,
                                 size_t commitment_len, const HFr* point, const HFr& value, Transcript& tr) {
  const SparkLayout lay{cc};
  std::vector<HG1> comms = argument_read_commitment_blob("spark", commitment, commitment_len, lay.committed());
  spark_header(tr, n, l, cc, comms, point);
  {
    const std::vector<HG1> block = lasso_read_commitments(tr, cc);
    comms.insert(comms.end(), block.begin(), block.end());
  }
  const HFr v = tr.read_field_element();
  if (v != value) throw Error(LH_ERR_INVALID_SNARK, "spark: the proof is of another value");
  const std::pair<HFr, std::vector<HFr>> sc = sum_check_verify(LH_SC_EVALUATIONS, n, cc + 1, v, tr);
  const std::vector<HFr>& r_z = sc.second;
  const std::vector<HFr> at_rz = tr.read_field_elements(cc + 1);
  HFr prod = HFr::one();
  for (const HFr& x : at_rz) prod = prod * x;
  if (prod != sc.first) throw Error(LH_ERR_INVALID_SNARK, "spark: sum-check final evaluation mismatch");
  const HFr gamma = tr.squeeze_challenge(), tau = tr.squeeze_challenge();
  std::vector<size_t> depths(4 * cc, n);
  for (size_t b = 2 * cc; b < 4 * cc; b++) depths[b] = l;
  std::vector<GpClaim> claims;
  const std::vector<HFr> roots = verify_grand_product(depths, tr, claims);  // RS_j, WS_j .., Init_j, Final_j ..
  for (size_t j = 0; j < cc; j++)
    if (roots[2 * cc + 2 * j] * roots[2 * j + 1] != roots[2 * j] * roots[2 * cc + 2 * j + 1])
      throw Error(LH_ERR_INVALID_SNARK, "spark: dimension " + std::to_string(j) + ": Init*WS != RS*Final");
  const std::vector<HFr>&r_N = claims[0].point, &r_M = claims[2 * cc].point;
  const std::vector<HFr> at_leaves = tr.read_field_elements(4 * cc);  // dim_j | read_ts_j | E_j at r_N, final_cts_j at r_M
  const Fingerprint h{gamma, tau};
  const HFr one = HFr::one(), id_M = identity_eval(r_M);
  for (size_t j = 0; j < cc; j++) {
    // the memory's extension in closed form: T_j~(r_M) = eq(r_M, r_j) - the verifier never sees a table
    const HFr rs = h(at_leaves[j], at_leaves[2 * cc + j], at_leaves[cc + j]);
    const HFr init = h(id_M, host_eq_xy_eval(r_M.data(), point + j * l, l), HFr::zero());
    if (claims[2 * j].claim != rs || claims[2 * j + 1].claim != rs + one || claims[2 * cc + 2 * j].claim != init ||
        claims[2 * cc + 2 * j + 1].claim != init + at_leaves[3 * cc + j])
      throw Error(LH_ERR_INVALID_SNARK, "spark: dimension " + std::to_string(j) + ": leaf claim mismatch");
  }
  std::vector<HFr> points;
  lasso_append_points(points, {&r_z, &r_N, &r_M}, nv);
  const std::vector<lh_evaluation> evs = spark_evaluations(lay, at_rz, at_leaves);
  pcs.batch_verify(nv, comms.data(), comms.size(), points.data(), 3, evs.data(), evs.size(), tr);
}
void spark_verify(const PcsVerifier& pcs, size_t n, size_t l, size_t cc, const uint8_t* commitment, size_t commitment_len,
                  const HFr* point, const HFr& value, Transcript& tr) {
  const size_t nv = spark_check(n, l, cc);
  LH_REQUIRE(commitment != nullptr && point != nullptr, LH_ERR_ARG, "null argument: commitment or point");
  argument_pcs_check(pcs, "spark");
  argument_verdict("spark", [&] { spark_verify_checked(pcs, n, l, cc, nv, commitment, commitment_len, point, value, tr); });
}

}  // namespace lh
