// Read-write memory checking: a stand-alone argument for RAM traces.  A trace of loads and stores over a mutable memory is
// consistent - every read returns the last value written to its cell - iff
//   Init u WS = RS u Final   as multisets of (address, value, time) triples, and every read's time precedes its own.
// The multiset identity is one grand-product GKR over four trees of fingerprints (gkr.cpp prove_grand_product), the order of
// the times a LogUp range check of the differences i - rt[i] in [0, 2^n) by one fractional sum-check over two fractions
// (prove_fractional_sum_check) with the identity table in closed form.  The reference holds no such argument; protocol and
// transcript schedule are specified in tests/memcheck_ref.py and reproduced here byte for byte.  Written against the PCS
// description (host.hpp Pcs / PcsVerifier), as logup.cpp is.
#include <algorithm>
#include "host.hpp"

namespace lh {

namespace {
// The two layouts of the argument.  PLAIN (tests/memcheck_ref.py): the image is public - host words or none - and the verifier
// folds it.  SEGMENT (tests/memcheck_segment_ref.py): the image is the committed column iv, opened at r_M beside fv.
constexpr size_t MAX_POLYS = 8, MAX_OPENINGS = 9;
struct MemcheckLayout {
  size_t num_polys, num_openings;
  size_t addr, rv, wv, rt, fv, ft, m, iv;  // places in the commitment block (iv: MAX_POLYS when there is none)
  // (poly, point) of the opened evaluations in the order they are written; points: 0 = r_N, 1 = r_M, 2 = x
  uint32_t openings[MAX_OPENINGS][2];
  size_t fv_at;  // the place of fv(r_M) among the evaluations; ft(r_M), rt(x), m(x) follow it, iv(r_M) is directly before it
};
// commitment order: addr, rv, wv, rt, fv, ft, m
constexpr MemcheckLayout PLAIN = {7, 8, 0, 1, 2, 3, 4, 5, 6, MAX_POLYS,
                                  {{0, 0}, {1, 0}, {2, 0}, {3, 0}, {4, 1}, {5, 1}, {3, 2}, {6, 2}, {0, 0}}, 4};
// commitment order: addr, rv, wv, iv, fv, rt, ft, m
constexpr MemcheckLayout SEGMENT = {8, 9, 0, 1, 2, 5, 4, 6, 7, 3,
                                    {{0, 0}, {1, 0}, {2, 0}, {5, 0}, {3, 1}, {4, 1}, {6, 1}, {5, 2}, {7, 2}}, 5};
constexpr size_t SEGMENT_HEADER = 2;  // the third header element of a segment proof (PLAIN: has_init in {0, 1})

void memcheck_header(Transcript& tr, size_t n, size_t l, size_t tag) {
  for (size_t v : {n, l, tag}) tr.common_field_element(HFr::from_u64(v));
}
std::vector<lh_evaluation> memcheck_evaluations(const MemcheckLayout& L, const std::vector<HFr>& vals) {
  std::vector<lh_evaluation> evs;
  for (size_t i = 0; i < vals.size(); i++) evs.push_back(make_evaluation(L.openings[i][0], L.openings[i][1], &vals[i]));
  return evs;
}
}  // namespace

size_t memcheck_check(size_t n, size_t l, bool has_init) {
  LH_REQUIRE(n >= 1 && n < 31, LH_ERR_ARG, "memcheck: num_vars out of range (1 to 30)");
  // (with an image the verifier folds its 2^mem_vars host words)
  LH_REQUIRE(!has_init || (l >= 1 && l <= (size_t)LH_MEMCHECK_MAX_INIT_VARS), LH_ERR_ARG,
             "memcheck: mem_vars out of range with an initial image (1 to " + std::to_string(LH_MEMCHECK_MAX_INIT_VARS) + ")");
  LH_REQUIRE(l >= 1 && l < 31, LH_ERR_ARG, "memcheck: mem_vars out of range (1 to 30)");
  return std::max(n, l);
}

static void memcheck_trace_check(const lh_memcheck_trace& trace) {
  LH_REQUIRE(trace.d_addr != nullptr, LH_ERR_ARG, "null argument: d_addr of the trace");
  LH_REQUIRE(trace.d_rv != nullptr, LH_ERR_ARG, "null argument: d_rv of the trace");
  LH_REQUIRE(trace.d_wv != nullptr, LH_ERR_ARG, "null argument: d_wv of the trace");
}
// the image on the device (arena memory of the caller's scope), null without one
static const uint32_t* memcheck_upload(Ctx& c, const uint32_t* init, size_t M) {
  if (!init) return nullptr;
  uint32_t* d = c.arena.alloc_n<uint32_t>(M);
  LH_HIP(hipMemcpyAsync(d, init, M * sizeof(uint32_t), hipMemcpyHostToDevice, c.stream));
  return d;
}

bool memcheck_witness(Ctx& c, const lh_memcheck_trace& trace, size_t n, size_t l, const uint32_t* init, uint32_t* d_rt,
                      uint32_t* d_fv, uint32_t* d_ft, uint32_t* d_m) {
  memcheck_check(n, l, init != nullptr);
  memcheck_trace_check(trace);
  ArenaScope scope(c.arena);
  const uint32_t* d_init = memcheck_upload(c, init, (size_t)1 << l);
  const bool ok = k_memcheck_trace(c, trace.d_addr, trace.d_rv, trace.d_wv, n, l, d_init, d_rt, d_fv, d_ft);
  k_memcheck_m(c, d_rt, (size_t)1 << n, d_m);
  c.sync();  // (the image's arena memory goes back with this scope)
  return ok;
}

size_t memcheck_segment_check(size_t n, size_t l) { return memcheck_check(n, l, false); }  // (no host fold: the limits without an image)

// what a segment proof adds to the plain one: the image as a device column to commit, and where the final values go
struct MemcheckSegment {
  const uint32_t* d_image;
  uint32_t* d_final;  // (or null)
};
// seg null: the plain argument over the public image `init`; else `init` is null and the image is seg->d_image
static void memcheck_prove_with(Ctx& c, const Pcs& pcs, const lh_memcheck_trace& trace, size_t n, size_t l, const uint32_t* init,
                                const MemcheckSegment* seg, Transcript& tr) {
  const MemcheckLayout& L = seg ? SEGMENT : PLAIN;
  const size_t nv = seg ? memcheck_segment_check(n, l) : memcheck_check(n, l, init != nullptr);
  memcheck_trace_check(trace);
  if (seg) LH_REQUIRE(seg->d_image != nullptr, LH_ERR_ARG, "null argument: d_image of the segment");
  argument_not_sharded(c, "memcheck");
  argument_pcs_check(pcs, nv, "memcheck", false);  // (every poly is a u32 column: nothing goes through batch_commit)
  const size_t N = (size_t)1 << n, M = (size_t)1 << l;
  open_precommit_cancel(c);
  ArenaScope scope(c.arena);
  EqHalfScope eq_scope(c);  // (the opening shares eq tables of its points: arena memory of this scope)

  // ---- 0/1: header; the witness (one flag readback); ONE block of seven commitments (a segment: eight, the image among
  // them), every column a 32-bit MSM over its own length (commit_u32_columns)
  memcheck_header(tr, n, l, seg ? SEGMENT_HEADER : (size_t)(init != nullptr));
  const uint32_t* d_init = seg ? seg->d_image : memcheck_upload(c, init, M);
  uint32_t* rt = c.arena.alloc_n<uint32_t>(N);
  uint32_t* fv = c.arena.alloc_n<uint32_t>(M);
  uint32_t* ft = c.arena.alloc_n<uint32_t>(M);
  uint32_t* m = c.arena.alloc_n<uint32_t>(N);
  if (!k_memcheck_trace(c, trace.d_addr, trace.d_rv, trace.d_wv, n, l, d_init, rt, fv, ft))
    throw Error(LH_ERR_INVALID_SNARK, "Invalid memory trace");
  k_memcheck_m(c, rt, N, m);
  const size_t num_polys = L.num_polys;
  const uint32_t* col[MAX_POLYS] = {};
  size_t len[MAX_POLYS] = {};
  auto place = [&](size_t at, const uint32_t* column, size_t length) { col[at] = column, len[at] = length; };
  place(L.addr, trace.d_addr, N), place(L.rv, trace.d_rv, N), place(L.wv, trace.d_wv, N), place(L.rt, rt, N);
  place(L.fv, fv, M), place(L.ft, ft, M), place(L.m, m, N);
  if (seg) place(L.iv, d_init, M);
  uint32_t bits[MAX_POLYS];
  {
    std::vector<U32Column> cols;
    for (size_t i = 0; i < num_polys; i++) cols.push_back(U32Column{col[i], len[i]});
    lasso_write_commitments(tr, commit_u32_columns(c, pcs, nv, cols, bits));
  }

  // ---- 2: gamma, tau; the four trees' leaves in one launch (and, fused, the level above the large ones); the grand product
  const HFr gamma = tr.squeeze_challenge(), tau = tr.squeeze_challenge();
  const bool fused = c.opt.logup_fused_leaves != 0;
  std::vector<HFr> r_N, r_M;
  {
    MemoryTrees trees(1, n, false);  // (one memory; its write leaves are no read leaves + 1)
    const MemoryTrees::Memory t = trees.add(c, 0, N, l, fused && n >= GP_LEVEL_UP_MIN_VARS, false, fused && l >= GP_LEVEL_UP_MIN_VARS);
    const MemcheckLeaves a = {{{col[L.addr], col[L.rv], col[L.rt], col[L.wv]}, {d_init, col[L.fv], col[L.ft], nullptr}},
                              {{t.rs, t.ws}, {t.init, t.fin}},
                              {{t.rs_up, t.ws_up}, {t.init_up, t.fin_up}},
                              {0, 0}};
    k_memcheck_leaves(c, a, n, l, dev(gamma), dev(gamma * gamma), dev(tau));
    const GrandProductResult gp = trees.prove(c, tr);
    r_N = gp.points[0], r_M = gp.points[2];
  }

  // ---- 3: delta; the range check i - rt[i] in [0, 2^n): sum_i 1 / (delta + i - rt[i]) = sum_d m[d] / (delta + d)
  const HFr delta = tr.squeeze_challenge();
  std::vector<HFr> x;
  {
    const bool up = fused && n >= 2;  // (one variable: the leaves are the top layer)
    MemcheckRangeLeaves a;
    memset(&a, 0, sizeof(a));
    a.rt = rt, a.m = m;
    a.ones = c.arena.alloc_n<Fr>(N), a.q0 = c.arena.alloc_n<Fr>(N), a.p1 = c.arena.alloc_n<Fr>(N), a.q1 = c.arena.alloc_n<Fr>(N);
    if (up) {
      a.p0_up = c.arena.alloc_n<Fr>(N / 2), a.q0_up = c.arena.alloc_n<Fr>(N / 2);
      a.p1_up = c.arena.alloc_n<Fr>(N / 2), a.q1_up = c.arena.alloc_n<Fr>(N / 2);
    }
    k_memcheck_range_leaves(c, a, n, up, dev(delta));
    const Fr* ps[2] = {a.ones, a.p1};
    const Fr* qs[2] = {a.q0, a.q1};
    const Fr* p_up[2] = {a.p0_up, a.p1_up};
    const Fr* q_up[2] = {a.q0_up, a.q1_up};
    x = prove_fractional_sum_check(c, 2, n, nullptr, nullptr, ps, qs, tr, up ? p_up : nullptr, up ? q_up : nullptr).x;
  }

  // ---- 4: the eight evaluations (a segment: nine, iv(r_M) before fv(r_M)), every column against the eq table of its point
  std::vector<HFr> vals(L.num_openings);
  auto evaluate = [&](const std::vector<HFr>& point, std::vector<size_t> polys, size_t first) {
    std::vector<const uint32_t*> cols;
    for (size_t i : polys) cols.push_back(col[i]);
    evaluate_u32_columns(c, cols.data(), cols.size(), point.data(), point.size(), vals.data() + first);
  };
  evaluate(r_N, {L.addr, L.rv, L.wv, L.rt}, 0);
  if (seg) evaluate(r_M, {L.iv, L.fv, L.ft}, L.fv_at - 1);
  else evaluate(r_M, {L.fv, L.ft}, L.fv_at);
  evaluate(x, {L.rt, L.m}, L.fv_at + 2);
  tr.write_field_elements(vals);

  // ---- 5: ONE batch opening over nv variables; every poly goes as its 32-bit column (mkzg.cpp all_small).  Nothing is
  // committed ahead - no Pcs::precommit call, the opening builds its column plan itself; the bytes do not depend on the route
  std::vector<const Fr*> polys(num_polys, nullptr);
  std::vector<SmallPoly> small(num_polys);
  for (size_t i = 0; i < num_polys; i++) small[i] = SmallPoly{col[i], len[i], bits[i]};
  std::vector<HFr> points;
  lasso_append_points(points, {&r_N, &r_M, &x}, nv);
  const std::vector<lh_evaluation> evs = memcheck_evaluations(L, vals);
  pcs.batch_open(nv, polys.data(), polys.size(), points.data(), 3, evs.data(), evs.size(), tr, small.data());
  // (behind the opening, the image's last reader: d_final may be the image's own memory)
  if (seg && seg->d_final) LH_HIP(hipMemcpyAsync(seg->d_final, fv, M * sizeof(uint32_t), hipMemcpyDeviceToDevice, c.stream));
}
void memcheck_prove(Ctx& c, const Pcs& pcs, const lh_memcheck_trace& trace, size_t n, size_t l, const uint32_t* init,
                    Transcript& tr) {
  memcheck_prove_with(c, pcs, trace, n, l, init, nullptr, tr);
}
void memcheck_prove_segment(Ctx& c, const Pcs& pcs, const lh_memcheck_trace& trace, size_t n, size_t l, const uint32_t* d_image,
                            uint32_t* d_final, Transcript& tr) {
  const MemcheckSegment seg = {d_image, d_final};
  memcheck_prove_with(c, pcs, trace, n, l, nullptr, &seg, tr);
}

void memcheck_replay(Ctx& c, const lh_memcheck_ops& ops, size_t n, size_t l, const uint32_t* d_image, uint32_t* d_rv, uint32_t* d_wv,
                     uint32_t* d_final) {
  memcheck_check(n, l, false);
  LH_REQUIRE(ops.d_addr != nullptr, LH_ERR_ARG, "null argument: d_addr of the operations");
  LH_REQUIRE(ops.d_store != nullptr, LH_ERR_ARG, "null argument: d_store of the operations");
  LH_REQUIRE(ops.d_val != nullptr, LH_ERR_ARG, "null argument: d_val of the operations");
  if (!k_memcheck_replay(c, ops.d_addr, ops.d_store, ops.d_val, n, l, d_image, d_rv, d_wv, d_final))
    throw Error(LH_ERR_INVALID_SNARK, "Invalid memory trace");
}

// segment: the image is the proof's column iv - its opened value stands where the plain verifier folds `init` (null then) -
// and the commitments of iv and fv are handed back
static void memcheck_verify_checked(const PcsVerifier& pcs, size_t n, size_t l, size_t nv, const uint32_t* init, Transcript& tr,
                                    HG1* segment) {
  const MemcheckLayout& L = segment ? SEGMENT : PLAIN;
  memcheck_header(tr, n, l, segment ? SEGMENT_HEADER : (size_t)(init != nullptr));
  const std::vector<HG1> comms = lasso_read_commitments(tr, L.num_polys);
  const HFr gamma = tr.squeeze_challenge(), tau = tr.squeeze_challenge();
  std::vector<GpClaim> claims;
  const std::vector<HFr> roots = verify_grand_product({n, n, l, l}, tr, claims);  // RS, WS, Init, Final
  if (roots[2] * roots[1] != roots[0] * roots[3]) throw Error(LH_ERR_INVALID_SNARK, "memcheck: Init*WS != RS*Final");
  const std::vector<HFr>&r_N = claims[0].point, &r_M = claims[2].point;
  const HFr delta = tr.squeeze_challenge();
  const FracVerifyResult fr = verify_fractional_sum_check(2, n, nullptr, nullptr, tr);
  if (!logup_roots_cancel(fr.p_0s[0], fr.q_0s[0], fr.p_0s[1], fr.q_0s[1]))  // the LogUp identity on the roots
    throw Error(LH_ERR_INVALID_SNARK, "memcheck: the fractions do not sum to zero");
  // addr, rv, wv, rt at r_N; (a segment: iv,) fv, ft at r_M; rt, m at x
  const std::vector<HFr> v = tr.read_field_elements(L.num_openings);
  const HFr &fv_e = v[L.fv_at], &ft_e = v[L.fv_at + 1], &rt_x = v[L.fv_at + 2], &m_x = v[L.fv_at + 3];
  const Fingerprint h{gamma, tau};
  const HFr one = HFr::one(), id_N = identity_eval(r_N), id_M = identity_eval(r_M), id_x = identity_eval(fr.x);
  // (the image's extension at r_M: one fold over its 2^l words)
  const HFr init_e = segment ? v[L.fv_at - 1]
                     : init  ? host_table_eval(l, r_M, [&](size_t a) { return HFr::from_u64(init[a]); })
                             : HFr::zero();
  if (claims[0].claim != h(v[0], v[1], v[3]) || claims[1].claim != h(v[0], v[2], id_N + one) ||
      claims[2].claim != h(id_M, init_e, HFr::zero()) || claims[3].claim != h(id_M, fv_e, ft_e))
    throw Error(LH_ERR_INVALID_SNARK, "memcheck: leaf claim mismatch");
  if (fr.p_xs[0] != one || fr.q_xs[0] != delta + id_x - rt_x || fr.p_xs[1] != HFr::zero() - m_x || fr.q_xs[1] != delta + id_x)
    throw Error(LH_ERR_INVALID_SNARK, "memcheck: range leaf claim mismatch");
  std::vector<HFr> points;
  lasso_append_points(points, {&r_N, &r_M, &fr.x}, nv);
  const std::vector<lh_evaluation> evs = memcheck_evaluations(L, v);
  pcs.batch_verify(nv, comms.data(), comms.size(), points.data(), 3, evs.data(), evs.size(), tr);
  if (segment) segment[0] = comms[L.iv], segment[1] = comms[L.fv];
}
void memcheck_verify(const PcsVerifier& pcs, size_t n, size_t l, const uint32_t* init, Transcript& tr) {
  const size_t nv = memcheck_check(n, l, init != nullptr);
  argument_pcs_check(pcs, "memcheck");
  argument_verdict("memcheck", [&] { memcheck_verify_checked(pcs, n, l, nv, init, tr, nullptr); });
}
void memcheck_verify_segment(const PcsVerifier& pcs, size_t n, size_t l, Transcript& tr, HG1* image_commitment,
                             HG1* final_commitment) {
  const size_t nv = memcheck_segment_check(n, l);
  argument_pcs_check(pcs, "memcheck");
  HG1 linked[2];
  argument_verdict("memcheck", [&] { memcheck_verify_checked(pcs, n, l, nv, nullptr, tr, linked); });
  if (image_commitment) *image_commitment = linked[0];
  if (final_commitment) *final_commitment = linked[1];
}

}  // namespace lh
