// Lasso lookup argument prover (Surge sum-check + offline memory checking by grand products).
// The reference snapshot holds no Lasso code (README.md:1-9 only); the protocol and
// transcript schedule are specified in oracle/pyref/lasso.py and reproduced here byte for byte.
#include <algorithm>
#include <chrono>
#include "host.hpp"

namespace lh {

static double now_ms() {
  using namespace std::chrono;
  return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}

// Commitment framing of the Lasso argument (oracle/pyref/lasso.py write_commitments / read_commitments).  A committed
// column that is identically zero commits to the identity - the high-limb dim of a 32-bit range check whose values are
// all below 2^16, read_ts when the indices are pairwise distinct - and the reference's transcript cannot encode the
// identity (util/transcript.rs:172-179,216-219).  So: ONE field element whose bit i says that commitment i is the
// identity, then the other commitments in order; only calls every TranscriptWrite / TranscriptRead offers.
// Commitments of `chunks` points (Pcs::chunks, Hyrax's rows): the count * chunks points are flattened commitment-major
// and framed by ceil(total / 63) mask elements written FIRST, mask k covering the positions 63 k .. 63 k + 62 - for
// chunks = 1 (count <= 63) exactly the one-mask framing above.
void lasso_write_commitments(Transcript& tr, const std::vector<HG1>& comms, size_t chunks) {
  LH_REQUIRE(chunks >= 1 && comms.size() % chunks == 0 && comms.size() / chunks < 64, LH_ERR_ARG,
             "lasso: too many commitments for the identity mask");
  for (size_t k = 0; 63 * k < comms.size(); k++) {
    uint64_t mask = 0;
    for (size_t i = 0; i < 63 && 63 * k + i < comms.size(); i++)
      if (comms[63 * k + i].is_identity()) mask |= (uint64_t)1 << i;
    tr.write_field_element(HFr::from_u64(mask));
  }
  for (const HG1& cm : comms)
    if (!cm.is_identity()) tr.write_commitment(cm);
}

std::vector<HG1> lasso_read_commitments(Transcript& tr, size_t count, size_t chunks) {
  LH_REQUIRE(count < 64 && chunks >= 1, LH_ERR_ARG, "lasso: too many commitments for the identity mask");
  const size_t total = count * chunks;
  std::vector<uint64_t> masks;
  for (size_t k = 0; 63 * k < total; k++) {
    const HFr m = tr.read_field_element();
    uint64_t canon[4];
    m.to_canonical(canon);
    const size_t width = std::min<size_t>(63, total - 63 * k);
    if (canon[1] || canon[2] || canon[3] || (canon[0] >> width))
      throw Error(LH_ERR_INVALID_SNARK, "lasso: commitment mask out of range");
    masks.push_back(canon[0]);
  }
  std::vector<HG1> comms(total);
  for (size_t i = 0; i < total; i++)
    comms[i] = (masks[i / 63] >> (i % 63)) & 1 ? HG1{host::Fq::zero(), host::Fq::zero()} : tr.read_commitment();
  return comms;
}

void lasso_check_table(const lh_lasso_table& tb) {
  const size_t cc = tb.num_chunks, l = tb.chunk_bits, alpha = tb.num_memories;
  LH_REQUIRE(cc >= 1 && cc <= LH_LASSO_MAX_CHUNKS, LH_ERR_ARG, "lasso: bad num_chunks");
  LH_REQUIRE(alpha >= 1 && alpha <= LH_LASSO_MAX_MEMORIES, LH_ERR_ARG, "lasso: bad num_memories");
  LH_REQUIRE(8 * alpha + 1 <= (size_t)SC_MAX_TABLES, LH_ERR_ARG, "lasso: too many memories for one GKR batch");
  LH_REQUIRE(l >= 1 && l < 31, LH_ERR_ARG, "lasso: need at least one variable");
  LH_REQUIRE(tb.num_terms >= 1 && tb.num_terms <= LH_LASSO_MAX_TERMS, LH_ERR_ARG, "lasso: bad g term count");
  for (size_t i = 0; i < alpha; i++) {
    LH_REQUIRE(tb.memory_chunk[i] < cc, LH_ERR_ARG, "lasso: memory chunk out of range");
    if (subtable_is_custom(tb.memory_subtable[i])) {  // (registered: its own size, odd or even)
      subtable_require(tb.memory_subtable[i], l);
      continue;
    }
    LH_REQUIRE(tb.memory_subtable[i] < LH_SUBTABLE_KINDS, LH_ERR_ARG, "lasso: unknown subtable");
    if (tb.memory_subtable[i] != LH_SUBTABLE_IDENTITY)
      LH_REQUIRE(l % 2 == 0, LH_ERR_ARG, "lasso: bitwise subtables need an even chunk_bits");
  }
  for (uint32_t m = 0; m < tb.num_terms; m++) {
    LH_REQUIRE(tb.g_num_factors[m] >= 1 && tb.g_num_factors[m] <= LH_SC_MAX_FACTORS, LH_ERR_ARG, "lasso: bad g term");
    for (int k = 0; k < tb.g_num_factors[m]; k++)
      LH_REQUIRE(tb.g_factor[m][k] < alpha, LH_ERR_ARG, "lasso: g factor out of range");
  }
}

// Access counters of a sharded proof: read_ts[k] = number of earlier lookups - in the GLOBAL lookup order - of the same
// address, final_cts[a] = number of lookups of a.  rts[j]: this rank's shard (2^(n - rho)), fcs[j]: replicated (2^l).
// No rank ever holds a whole column: the lookups are repartitioned by address (owner = address mod R), the owner sorts
// the keys it receives and ranks every lookup inside its address run, the ranks travel back the same way.  All chunk
// columns go together: per PROOF two personalised exchanges of ~cc 2^(n - rho) entries per rank (4 B out - kernels_poly.hip:
// the key needs neither the sender nor the low index bits -, 4 B back), one host all-gather of the segment boundaries and
// one all-gather of the cc 2^l / R counts of every owner.  Work and traffic per rank shrink with R (a column that hits one
// address only degenerates to the single-GPU sort on that address's owner).
static void lasso_counters_sharded(Ctx& c, const Shard& sh, const uint32_t* const* d_dims_local, size_t cc, size_t n, size_t l,
                                   uint32_t* const* rts, uint32_t* const* fcs) {
  const size_t R = sh.R, me = sh.rank, M = (size_t)1 << l, NL = (size_t)1 << (n - sh.rho);
  const size_t m_loc = std::max<size_t>(M >> sh.rho, 1), R1 = R + 1;
  unsigned a_bits = 0;
  while (((size_t)1 << a_bits) < m_loc) a_bits++;
  const unsigned hi_bits = (unsigned)(n - sh.rho - sh.j);  // the local index bits above the shard bits
  ArenaScope scope(c.arena);
  uint32_t* sidx_all = c.arena.alloc_n<uint32_t>(cc * NL);
  uint32_t* send_all = c.arena.alloc_n<uint32_t>(cc * NL);
  std::vector<uint32_t*> sidx(cc), send(cc);
  for (size_t q = 0; q < cc; q++) sidx[q] = sidx_all + q * NL, send[q] = send_all + q * NL;
  // everybody's segment boundaries: starts[s][q][o] = where, in rank s's send buffer of column q, the lookups for owner o
  // begin - and everybody's verdict on its own shard: an index out of range on ANY rank fails the prove on EVERY rank,
  // after the exchange (a rank that threw on its own would leave its peers waiting in this collective)
  const size_t W = cc * R1 + 1;
  std::vector<uint32_t> start(W), starts(W * R);
  bool bad = false;
  k_cs_partition(c, d_dims_local, cc, NL, M, (unsigned)sh.rho, (unsigned)sh.j, hi_bits, sidx.data(), send.data(), start.data(), &bad);
  start[cc * R1] = bad ? 1u : 0u;
  comm_all_gather_host(c, start.data(), starts.data(), W * sizeof(uint32_t));
  for (size_t s = 0; s < R; s++)
    LH_REQUIRE(!starts[s * W + cc * R1], LH_ERR_ARG, "lasso: chunk index out of range (>= 2^chunk_bits)");
  auto seg = [&](size_t s, size_t q, size_t o) { return (size_t)(starts[s * W + q * R1 + o + 1] - starts[s * W + q * R1 + o]); };
  std::vector<size_t> s_off(cc * R), s_cnt(cc * R), r_off(cc * R), r_cnt(cc * R), peer_off(cc * R), back_peer_off(cc * R, 0);
  std::vector<size_t> recv_total(cc, 0);
  size_t recv_max = 0, recv_sum = 0;
  for (size_t q = 0; q < cc; q++) {
    for (size_t p = 0; p < R; p++) {
      s_off[q * R + p] = start[q * R1 + p], s_cnt[q * R + p] = seg(me, q, p);
      r_off[q * R + p] = recv_total[q], r_cnt[q * R + p] = seg(p, q, me), peer_off[q * R + p] = starts[p * W + q * R1 + me];
      recv_total[q] += r_cnt[q * R + p];
      // (where, in owner p's return buffer, the segment for this rank begins: the lookups of ranks 0..me-1 come first)
      for (size_t s = 0; s < me; s++) back_peer_off[q * R + p] += seg(s, q, p);
    }
    recv_sum += recv_total[q];
    for (size_t o = 0; o < R; o++) {  // (the largest receive buffer of any owner and column: the stride of the way back)
      size_t t = 0;
      for (size_t s = 0; s < R; s++) t += seg(s, q, o);
      recv_max = std::max(recv_max, t);
    }
  }
  recv_max = std::max<size_t>(recv_max, 1);
  uint32_t* recv_all = c.arena.alloc_n<uint32_t>(std::max<size_t>(recv_sum, 1));
  uint32_t* ret_all = c.arena.alloc_n<uint32_t>(cc * recv_max);
  uint32_t* back_all = c.arena.alloc_n<uint32_t>(cc * NL);
  uint32_t* counts = c.arena.alloc_n<uint32_t>(cc * m_loc);
  std::vector<uint32_t*> recv(cc), ret(cc), back(cc);
  {
    size_t off = 0;
    for (size_t q = 0; q < cc; q++) recv[q] = recv_all + off, off += recv_total[q], ret[q] = ret_all + q * recv_max, back[q] = back_all + q * NL;
  }
  std::vector<const void*> csend(send.begin(), send.end()), cret(ret.begin(), ret.end());
  std::vector<void*> vrecv(recv.begin(), recv.end()), vback(back.begin(), back.end());
  comm_all_to_all_multi(c, cc, csend.data(), s_off.data(), s_cnt.data(), vrecv.data(), r_off.data(), r_cnt.data(), peer_off.data(),
                        send_all, NL, sizeof(uint32_t));
  // the owner's side: rank inside the address run, per-address totals
  std::vector<const uint32_t*> crecv(recv.begin(), recv.end());
  k_cs_rank(c, crecv.data(), recv_total.data(), cc, hi_bits, a_bits, m_loc, ret.data(), counts);
  // the ranks go back along the same segments (the send side of the way back is this rank's receive layout)
  comm_all_to_all_multi(c, cc, cret.data(), r_off.data(), r_cnt.data(), vback.data(), s_off.data(), s_cnt.data(),
                        back_peer_off.data(), ret_all, recv_max, sizeof(uint32_t));
  std::vector<const uint32_t*> cback(back.begin(), back.end()), csidx(sidx.begin(), sidx.end());
  k_cs_scatter(c, cback.data(), csidx.data(), cc, NL, rts);
  uint32_t* all_counts = c.arena.alloc_n<uint32_t>(cc * m_loc * R);
  comm_all_gather_dev(c, counts, all_counts, cc * m_loc * sizeof(uint32_t));
  k_cs_final(c, all_counts, cc, M, (unsigned)sh.rho, m_loc, fcs);
  c.sync();  // (the scope's buffers are released)
  c.route.v[RouteStats::SHARD_EXCHANGES] += 3;
}

// witness: access counters, subtable reads and (optionally) the lookup outputs a = g(E); arena memory of the caller's scope.
// Inside a sharded proof d_dims are this rank's shards of the lookup columns and so are read_ts / E / a; final_cts (2^l
// entries, l <= shard_bit + rho) is replicated.
LassoColumns lasso_witness_columns(Ctx& c, const lh_lasso_table& tb, size_t n, const uint32_t* const* d_dims, Fr** a_out,
                                   uint32_t** a_small_out, bool keep_sorted, const LassoColumns* reuse) {
  const size_t cc = tb.num_chunks, l = tb.chunk_bits, alpha = tb.num_memories;
  const Shard sh(c);
  const size_t N = (size_t)1 << (n - sh.rho), M = (size_t)1 << l;  // N: entries of this rank's columns
  LassoColumns w;
  w.rts.resize(cc), w.fcs.resize(cc), w.E.resize(alpha), w.T.assign(alpha, nullptr);
  w.tables = std::make_shared<SubtableOrders>(c, l);
  // reuse (a batch proof, not sharded): rts[j] / fcs[j] given say that chunk column j was counted for an earlier table
  std::vector<const uint32_t*> own_dims;
  std::vector<uint32_t*> own_rts, own_fcs;
  for (size_t j = 0; j < cc; j++) {
    if (reuse && reuse->rts[j]) {
      w.rts[j] = reuse->rts[j], w.fcs[j] = reuse->fcs[j];
      continue;
    }
    w.rts[j] = c.arena.alloc_n<uint32_t>(N);
    w.fcs[j] = c.arena.alloc_n<uint32_t>(M);
    own_dims.push_back(d_dims[j]), own_rts.push_back(w.rts[j]), own_fcs.push_back(w.fcs[j]);
  }
  // LH_SHARDED_COUNTERS_MIN_R=1 (tests): a world of one takes the repartitioned counters too (the personalised exchange
  // then has one peer, itself: the transport's point-to-point path on a one-GPU box)
  const size_t counters_min_r = (size_t)knob(Knob::SHARDED_COUNTERS_MIN_R);
  keep_sorted = keep_sorted && !(sh.on && sh.R >= counters_min_r);
  if (sh.on && sh.R >= counters_min_r) {
    LH_REQUIRE(own_dims.size() == cc, LH_ERR_ARG, "lasso: shared chunk columns inside a sharded prove");
    lasso_counters_sharded(c, sh, d_dims, cc, n, l, w.rts.data(), w.fcs.data());
  } else if (!own_dims.empty()) {
    if (keep_sorted)
      for (size_t j = 0; j < own_dims.size(); j++) {  // (one pair per column counted here, in their order)
        w.dim_sorted.push_back(c.arena.alloc_n<uint32_t>(N));
        w.dim_index.push_back(c.arena.alloc_n<uint32_t>(N));
      }
    // all chunk columns in one launch set, one bad-index readback (kernels_poly.hip)
    k_lasso_counters(c, own_dims.data(), own_dims.size(), N, M, own_rts.data(), own_fcs.data(),
                     keep_sorted ? w.dim_sorted.data() : nullptr, keep_sorted ? w.dim_index.data() : nullptr);
  }
  LassoG g;
  memset(&g, 0, sizeof(g));
  for (size_t i = 0; i < alpha; i++) {
    if (tb.memory_subtable[i] == LH_SUBTABLE_IDENTITY) {
      // E = dim entry by entry: the same column (read-only everywhere; the batch opening merges columns it is handed twice)
      w.E[i] = const_cast<uint32_t*>(d_dims[tb.memory_chunk[i]]);
    } else {
      w.E[i] = c.arena.alloc_n<uint32_t>(N);
      // (a registered kind: a gather from its entries, uploaded once per kind; the kernel masks the index)
      if (subtable_is_custom(tb.memory_subtable[i])) w.T[i] = w.tables->custom_table(tb.memory_subtable[i]);
      k_lasso_subtable_read(c, (int)tb.memory_subtable[i], (uint32_t)l, d_dims[tb.memory_chunk[i]], N, w.E[i], w.T[i]);
    }
    g.e[i] = w.E[i];
  }
  if (a_small_out) {
    // a 32-bit output column when g = sum coeff_t E_t with small coefficients and the largest value fits 32 bits
    *a_small_out = nullptr;
    LassoGSmall gs;
    memset(&gs, 0, sizeof(gs));
    gs.num_terms = tb.num_terms;
    bool ok = true;
    uint64_t max_val = 0;
    for (uint32_t m = 0; m < tb.num_terms && ok; m++) {
      uint64_t co = 0;
      const size_t i = tb.g_factor[m][0];
      const size_t ebits = lasso_subtable_bits(tb.memory_subtable[i], l);
      ok = tb.g_num_factors[m] == 1 && lasso_g_coeff_fits(tb, m, 32, &co) && ebits <= 32;
      if (!ok) break;
      max_val += co * (((uint64_t)1 << ebits) - 1);
      ok = max_val <= 0xffffffffull;
      gs.coeff[m] = (uint32_t)co;
      gs.fac[m] = (uint8_t)i;
    }
    if (ok) {
      for (size_t i = 0; i < alpha; i++) gs.e[i] = w.E[i];
      *a_small_out = c.arena.alloc_n<uint32_t>(N);
      k_lasso_output_small(c, gs, N, *a_small_out);
      if (a_out) *a_out = nullptr;
      return w;
    }
    // g with product terms (less_than / equal): bound = sum_m coeff_m prod_k (2^bits(E_f(m,k)) - 1) from the subtables'
    // widths; with LH_LASSO_PRODUCT_U32=1 a 32-bit column when every coefficient and the bound fit 32 bits (default 0: the
    // field-element column below - the proof bytes are the same)
    bool product_g = false;
    for (uint32_t m = 0; m < tb.num_terms; m++) product_g = product_g || tb.g_num_factors[m] > 1;
    if (product_g && knob(Knob::LASSO_PRODUCT_U32) != 0) {
      LassoGSmallProd gp;
      memset(&gp, 0, sizeof(gp));
      gp.num_terms = tb.num_terms;
      unsigned __int128 bound = 0;
      bool fits = true;
      for (uint32_t m = 0; m < tb.num_terms && fits; m++) {
        uint64_t co = 0;
        fits = lasso_g_coeff_fits(tb, m, 32, &co);
        unsigned __int128 term = co;  // (< 2^32, and every step below keeps it <= 2^32 * (2^32 - 1) < 2^128)
        for (int k = 0; k < tb.g_num_factors[m] && fits; k++) {
          const uint32_t eb = lasso_subtable_bits(tb.memory_subtable[tb.g_factor[m][k]], l);
          term *= ((uint64_t)1 << eb) - 1;  // (eb <= l < 31)
          fits = term <= 0xffffffffull;
          gp.fac[m][k] = tb.g_factor[m][k];
        }
        bound += term;
        fits = fits && bound <= 0xffffffffull;
        gp.coeff[m] = (uint32_t)co;
        gp.nfac[m] = tb.g_num_factors[m];
      }
      if (fits) {
        for (size_t i = 0; i < alpha; i++) gp.e[i] = w.E[i];
        *a_small_out = c.arena.alloc_n<uint32_t>(N);
        k_lasso_output_small_prod(c, gp, N, *a_small_out);
        w.a_bits = std::max(bit_length((uint64_t)bound), 1u);
        if (a_out) *a_out = nullptr;
        return w;
      }
    }
  }
  if (a_out) {
    g.num_terms = tb.num_terms;
    for (uint32_t m = 0; m < tb.num_terms; m++) {
      memcpy(&g.coeff[m], &tb.g_coeff[m], 32);
      g.nfac[m] = tb.g_num_factors[m];
      for (int k = 0; k < LH_SC_MAX_FACTORS; k++) g.fac[m][k] = tb.g_factor[m][k];
    }
    *a_out = c.arena.alloc_n<Fr>(N);
    k_lasso_output(c, g, N, *a_out);
  }
  return w;
}

// ------------------------------------------------------------------ steps shared by lasso_argue, lasso_prove and lasso_prove_batch
// (final_cts at r_M, and any column of fewer than two variables: evaluate_u32_columns, against the point's full eq table)
// u32 columns of n variables (this rank's shards inside a sharded proof: partial sums added over the ranks) evaluated at
// `point`: against the eq table of point[1..] (half the entries), which the sum-checks and the batch opening at that point
// use as well.  The eq table that stays cached for the opening is obtained OUTSIDE any inner ArenaScope.
// share_sums: from the columns' quad sums, which stay in the proof's table for the opening (quad_sums_evaluate).
static void lasso_evaluate_u32(Ctx& c, const uint32_t* const* cols, size_t count, const HFr* point, size_t n, bool shn, HFr* out,
                               bool share_sums = false) {
  if (n < 2) return evaluate_u32_columns(c, cols, count, point, n, out);
  const Fr* eq_half = eq_half_get(c, point, n, shn);
  const size_t N = (size_t)1 << (n - Shard(c).rho);
  if (share_sums) quad_sums_evaluate(c, cols, count, point, n, eq_half, out);
  else k_inner_products_small_half(c, cols, count, eq_half, N / 2, dev(point[0]), (Fr*)out);
  if (shn) comm_sum_fr(c, out, count);
}
// the expression of the linear Surge case: one term, table 0, coefficient one
static lh_sop lasso_one_term() {
  lh_sop e;
  memset(&e, 0, sizeof(e));
  const HFr one = HFr::one();
  e.num_terms = 1, e.num_factors[0] = 1;
  memcpy(&e.coeff[0], &one, 32);
  return e;
}
// appends g's terms to `e` over tables whose memory i is table mem_base + i; coefficients times *scale where given
static void lasso_append_g(lh_sop& e, const lh_lasso_table& tb, size_t mem_base = 0, const HFr* scale = nullptr) {
  for (uint32_t m = 0; m < tb.num_terms; m++) {
    const uint32_t t = e.num_terms++;
    const HFr co = scale ? lasso_g_coeff(tb, m) * *scale : lasso_g_coeff(tb, m);
    memcpy(&e.coeff[t], &co, 32);
    e.num_factors[t] = tb.g_num_factors[m];
    for (int k = 0; k < tb.g_num_factors[m]; k++) e.factor[t][k] = (uint8_t)(mem_base + tb.g_factor[m][k]);
  }
}

// Steps 2-7 of the argument (oracle/pyref/lasso.py argue): Surge sum-check, memory-checking grand products,
// evaluations.  The Fr tables hold at least 2^n (fcs_fr: 2^l) entries; `lap` (optional) receives phase boundaries,
// `trees_built` (optional) is prove_grand_product's.
LassoClaims lasso_argue(Ctx& c, const lh_lasso_table& tb, size_t n, const LassoColumns& w, const uint32_t* const* d_dims,
                        const Fr* a, const Fr* const* E_fr, Transcript& tr, const std::function<void(int)>& lap,
                        const uint32_t* a_small, const std::function<void()>& trees_built) {
  const LassoLayout lay(tb);
  const size_t cc = lay.cc, l = lay.l, alpha = lay.alpha;
  const bool linear_g = lay.linear_g;
  // inside a sharded proof (dev.hpp Shard) every n-variable column is this rank's shard (N entries); sums over a column -
  // evaluations, round messages - are partial sums added over the ranks; the 2^l-entry subtable side is replicated
  const Shard sh(c);
  const bool shn = sh.on;
  if (shn) LH_REQUIRE(sh.sharded(n) && l <= sh.j + sh.rho, LH_ERR_ARG, "lasso: shard geometry does not fit the table");
  const size_t N = (size_t)1 << (n - sh.rho), M = (size_t)1 << l;
  LassoClaims cl;
  // ---- 2-4: Surge primary sum-check
  cl.r = tr.squeeze_challenges(n);
  c.host_stamp("argue:squeezed");
  Fr a_sums[4];  // (k_inner_products_small_quads: the claim's two halves - and rounds 0 and 1 of the Surge sum-check over a)
  bool have_a_sums = false;
  // Where the batch opening will take its rounds 0 and 1 from the columns' quad sums (sc_open_column_rounds - a guess: the
  // opening may still decide otherwise, then the table below is simply not read), the evaluations at r_z and r_N are made
  // from those very sums, which stay in the proof's table (quad_sums_evaluate); Surge's round 0 leaves the entry of a at r.
  // (n >= l: the opening's points are these, not zero-padded ones.)  LH_OPEN_SHARE_SUMS=0: as before, for A/B.
  const bool share_sums = !shn && n >= 3 && n >= l && knob(Knob::OPEN_SHARE_SUMS) != 0 && sc_open_column_rounds(c, n, shn);
  if (a_small && !a && linear_g && !shn && n >= 3) {
    // against the eq table of r[1..] (half the entries), which the Surge sum-check and the batch opening at r use as well
    const Fr* eq_half = eq_half_get(c, cl.r.data(), n, shn);
    k_inner_products_small_quads(c, a_small, eq_half, N / 4, a_sums);
    const HFr r0 = cl.r[0];
    cl.v = (HFr::one() - r0) * hst(a_sums[0]) + r0 * hst(a_sums[1]);
    have_a_sums = true;
    // even = (1 - y1) S_0 + y1 S_2 and odd = (1 - y1) S_1 + y1 S_3 with y1 = r[1]: S_0 and S_1 from the kernel's four sums
    const HFr y1 = cl.r[1], n1 = HFr::one() - y1;
    if (share_sums && !n1.is_zero()) {
      const HFr inv = n1.inv();
      const HFr s4[4] = {(hst(a_sums[0]) - y1 * hst(a_sums[2])) * inv, (hst(a_sums[1]) - y1 * hst(a_sums[3])) * inv,
                         hst(a_sums[2]), hst(a_sums[3])};
      quad_sums_put(c, a_small, N, cl.r.data(), n, s4);
    }
  } else if (a_small) {
    lasso_evaluate_u32(c, &a_small, 1, cl.r.data(), n, shn, &cl.v);
  } else {
    cl.v = evaluate_polys(c, &a, 1, n, cl.r.data(), shn)[0];
  }
  tr.write_field_element(cl.v);
  SumCheckResult sc;
  if (linear_g) {
    // g linear (range / AND / XOR): the summand eq * sum_m coeff_m E_m IS eq * a entry by entry, and binding is linear
    // too, so the round messages of the sum-check over the alpha subtable-read columns are those of the sum-check over
    // the single output column a.  One table instead of alpha in every round; the evaluations E_i(r_z) the transcript
    // wants next are inner products of the 32-bit columns with eq(r_z).
    {
      ArenaScope scope(c.arena);
      const Fr* a_tab = a;
      ScU32 u32;
      ScOptions so;
      so.sum_is_exact = true, so.sharded = shn;
      if (!a_tab) {
        // no field-element view of the output column: the sum-check runs its first three rounds from the 32-bit column where
        // it can (a_sums above are rounds 0 and 1) and fills this table itself where it cannot (host.hpp ScU32)
        a_tab = c.arena.alloc_n<Fr>(N);
        u32.col = a_small;
        u32.have_sums = have_a_sums;
        if (have_a_sums) u32.odd = a_sums[1], u32.s2 = a_sums[2], u32.s3 = a_sums[3];
        so.u32 = &u32;
      }
      sc = sum_check_prove(c, LH_SC_EVALUATIONS, n, lasso_one_term(), &a_tab, 1, cl.r.data(), 1, cl.v, tr, so);
    }
    std::vector<const uint32_t*> cols(w.E.begin(), w.E.end());
    sc.evals.assign(alpha, HFr::zero());  // (the table of r_z[1..] stays for the batch opening at r_z)
    lasso_evaluate_u32(c, cols.data(), alpha, sc.challenges.data(), n, shn, sc.evals.data(), share_sums);
  } else {
    lh_sop surge;
    memset(&surge, 0, sizeof(surge));
    lasso_append_g(surge, tb);
    ScOptions so;
    so.sum_is_exact = true, so.sharded = shn;
    sc = sum_check_prove(c, LH_SC_EVALUATIONS, n, surge, E_fr, alpha, cl.r.data(), 1, cl.v, tr, so);
  }
  cl.r_z = sc.challenges;
  cl.e_rz = sc.evals;
  tr.write_field_elements(sc.evals);
  if (lap) lap(2);

  // ---- 5/6: memory-checking fingerprints and product trees
  HFr gamma = tr.squeeze_challenge();
  HFr tau = tr.squeeze_challenge();
  HFr gamma2 = gamma * gamma;
  {
    ArenaScope scope(c.arena);
    MemoryTrees trees(alpha, n);
    // (sharded: the level above the leaves must itself be held in shards, else it is exchanged by the tree builder)
    const bool fused_up = n >= GP_LEVEL_UP_MIN_VARS && (!shn || sh.sharded(n - 1)), ws_implicit = fused_up && n > l;
    for (size_t i = 0; i < alpha; i++) {
      const size_t j = tb.memory_chunk[i];
      const MemoryTrees::Memory m = trees.add(c, i, N, l, fused_up, ws_implicit);
      if (fused_up)  // the level above the leaves comes with them (no tree_up pass over the largest level)
        k_lasso_rw_leaves_up(c, d_dims[j], w.E[i], w.rts[j], N, dev(gamma), dev(gamma2), dev(tau), m.rs, m.ws, m.rs_up, m.ws_up);
      else
        k_lasso_rw_leaves(c, d_dims[j], w.E[i], w.rts[j], N, dev(gamma), dev(gamma2), dev(tau), m.rs, m.ws);
      k_lasso_if_leaves(c, (int)tb.memory_subtable[i], (uint32_t)l, w.fcs[j], M, dev(gamma), dev(gamma2), dev(tau), m.init, m.fin,
                        w.T.empty() ? nullptr : w.T[i]);
    }
    if (lap) lap(3);
    GrandProductResult gp = trees.prove(c, tr, trees_built);
    cl.r_N = gp.points[0];
    cl.r_M = gp.points[2 * alpha];
  }
  if (lap) lap(4);

  // ---- 7: evaluations at r_N / r_M: dim | read_ts | E, then final_cts - straight from the u32 columns (no
  // field-element views: 4 bytes read and 8 multiply-adds per entry)
  std::vector<const uint32_t*> at_n(d_dims, d_dims + cc);
  at_n.insert(at_n.end(), w.rts.begin(), w.rts.end());
  at_n.insert(at_n.end(), w.E.begin(), w.E.end());
  cl.ev_n.resize(at_n.size());
  lasso_evaluate_u32(c, at_n.data(), at_n.size(), cl.r_N.data(), n, shn, cl.ev_n.data(), share_sums);
  std::vector<const uint32_t*> at_l(w.fcs.begin(), w.fcs.end());
  cl.ev_l.resize(cc);
  evaluate_u32_columns(c, at_l.data(), cc, cl.r_M.data(), l, cl.ev_l.data());
  tr.write_field_elements(cl.ev_n);
  tr.write_field_elements(cl.ev_l);
  if (lap) lap(5);
  return cl;
}

// The scope of a prove (lasso_prove, lasso_prove_batch).  Its phase boundaries are EVENTS on the prover's stream (a
// hipStreamSynchronize at each of them drained the queue seven times per proof for the sake of a number nobody reads in
// production): lh_lasso_last_timing turns them into phase times when asked (Ctx::phase_times_resolve); lasso_ms[8], the
// total, is the host's wall clock.  Everything the prove allocates, caches and starts ends with it: arena memory, the shared
// eq tables and quad sums, the route counters of an earlier prove, a precommit still running.  The cancel on entry was the
// batch prover's, the one on exit the single prover's guard (a prove that fails on the way drops what it started); with
// no precommit pending either is a no-op, so each path gained one without effect.
struct LassoPhases {
  Ctx& c;
  const double t0 = now_ms();
  struct Start {  // (ahead of the scopes below)
    explicit Start(Ctx& c) {
      for (int k = 0; k < 8; k++) (void)c.phase_ev[k].get();  // (all of them exist before the first is recorded)
      c.phase_ev_pending = false;
      LH_HIP(hipEventRecord(c.phase_ev[0].get(), c.stream));
      c.comm_phase = 0;
      c.quad_sums.clear();  // (nothing of an earlier prove: the arena hands out the same pointers again)
    }
  } start;
  ArenaScope scope;
  EqHalfScope eq_scope;  // (the shared eq tables are arena memory of this scope)
  explicit LassoPhases(Ctx& c_) : c(c_), start(c_), scope(c_.arena), eq_scope(c_) {
    open_precommit_cancel(c);
    c.route = RouteStats();
  }
  ~LassoPhases() {
    open_precommit_cancel(c);
    c.comm_phase = 7;  // (collectives issued after the prove - or after it failed - count as outside)
  }
  void lap(int idx) {
    LH_HIP(hipEventRecord(c.phase_ev[idx + 1].get(), c.stream));
    c.comm_phase = idx + 1;
  }
  void done() {  // the prove went through: its times may be read
    c.lasso_ms[7] = 0;
    c.lasso_ms[8] = now_ms() - t0;
    c.phase_ev_pending = true;
  }
};

// One table's share of a commit batch (msm_batch): which jobs of the batch are its own and where their results go in its
// commitment list a | dim | read_ts | E | final_cts.  lasso_prove runs one table's jobs, lasso_prove_batch every table's in
// one batch; both build them here.
struct LassoCommitPlan {
  std::vector<size_t> job, slot;  // job[k]: index in the batch; slot[k]: position of its result in the table's commitments
  std::vector<HG1> second;        // per chunk: the second output of a packed read_ts pair (MsmJob::out_second points here)
  std::vector<size_t> second_of;  // chunks whose read_ts commitment comes back through `second`
  std::vector<size_t> dim_job;    // per chunk: the job of the batch that commits dim_j (this table's, or the one it shares)
};
// one table of a prove: lasso_prove works on one of these, lasso_prove_batch on K
struct LassoTable {
  const lh_lasso_table* tb = nullptr;
  LassoLayout lay;
  const uint32_t* const* dims = nullptr;  // the chunk columns (device)
  LassoColumns w;
  Fr* a = nullptr;  // the output column: as field elements, or (then a stays null) in its 32-bit form
  uint32_t* a_small = nullptr;
  std::vector<uint32_t> count_ors;  // OR of every final_cts column (bounds its read_ts column) where computed, else 0
  LassoCommitPlan plan;
  SmallLinear a_linear;  // a = sum_m coeff_m E_{f(m)} entry by entry (linear g): what lasso_open_columns points small[a] at
  LassoClaims cl;
  LassoTable(const lh_lasso_table& tb_, const uint32_t* const* dims_) : tb(&tb_), lay(tb_), dims(dims_), count_ors(lay.cc, 0) {}
};
// Appends the table's jobs to `jobs`: the output column only when g is not linear (a linear g's follows from the E
// commitments), dim (with the sorted columns of the access counters where kept), read_ts (two columns packed into one pass
// where their widths allow), E of the non-identity subtables (derived from dim's buckets where the route applies) and
// final_cts.  count_ors: OR of every final_cts column; computed here when the packing looks at it unless `ors_known`.
// shared_dim_job (optional, per chunk): >= 0 says that this chunk column, its counters and their commitments belong to an
// earlier table of the batch whose dim job that is - no dim / read_ts / final_cts job is made for it (the caller copies
// those three commitments), and a derived E names that job as its parent.
static void lasso_commit_jobs(Ctx& c, const Pcs& pcs, LassoTable& x, size_t n, size_t nv, bool ors_known, const int* shared_dim_job,
                              std::vector<MsmJob>& jobs) {
  const lh_lasso_table& tb = *x.tb;
  const LassoLayout& lay = x.lay;
  const LassoColumns& w = x.w;
  LassoCommitPlan& plan = x.plan;
  std::vector<uint32_t>& count_ors = x.count_ors;
  const uint32_t* const* d_dims = x.dims;
  const size_t cc = lay.cc, l = lay.l, alpha = lay.alpha;
  const Shard sh(c);
  const bool shn = sh.on;
  const size_t N = (size_t)1 << (n - sh.rho), M = (size_t)1 << l;
  const std::vector<uint32_t*>&rts = w.rts, &fcs = w.fcs, &E = w.E;
  auto shared = [&](size_t j) { return shared_dim_job != nullptr && shared_dim_job[j] >= 0; };
  const G1Affine* bases = shn ? pcs.shard_bases(nv) : pcs.commit_bases(nv);
  auto add_job = [&](size_t pos, const void* col, bool u32, size_t len) {
    plan.job.push_back(jobs.size());
    jobs.push_back(MsmJob{col, u32, bases, len});
    plan.slot.push_back(pos);
  };
  if (!lay.linear_g && x.a_small) {  // (product g with a 32-bit output column: a u32 job, every entry below 2^a_bits)
    add_job(lay.a(), x.a_small, true, N);
    jobs.back().known_bits = w.a_bits;
  } else if (!lay.linear_g) {
    add_job(lay.a(), x.a, false, N);
  }
  std::vector<size_t>& dim_job = plan.dim_job;
  dim_job.assign(cc, 0);
  size_t own = 0;  // (the sorted columns are kept for the chunks this table counted itself, in their order)
  for (size_t j = 0; j < cc; j++) {
    if (shared(j)) {
      dim_job[j] = (size_t)shared_dim_job[j];
      continue;
    }
    dim_job[j] = jobs.size(), add_job(lay.dim(j), d_dims[j], true, N);
    jobs.back().known_bits = (uint32_t)l;  // (the access counters rejected any index >= 2^l)
    if (!w.dim_sorted.empty()) {
      jobs.back().sorted_scalars = w.dim_sorted[own], jobs.back().sorted_index = w.dim_index[own];
      c.route.v[RouteStats::SORTED_REUSE]++;
    }
    own++;
  }
  // read_ts columns are small (a cell's access count): two of them share one pass over the points when their bit
  // lengths allow (MsmJob::pack_shift; the access counts bound the timestamps)
  plan.second.assign(cc, HG1());
  std::vector<HG1>& second = plan.second;
  {
    std::vector<uint32_t>& ors = count_ors;
    std::vector<const uint32_t*> cols(fcs.begin(), fcs.end());
    const bool pack_on = c.opt.lasso_pack_ts != 0;  // 0: one MSM pass per read_ts column (A/B measurements)
    if (!ors_known && pack_on && cc >= 2 && N >= ((size_t)1 << 12)) k_or_u32(c, cols.data(), cc, M, ors.data());
    for (size_t j = 0; j < cc; j++) {
      if (shared(j)) continue;
      const bool next = j + 1 < cc && !shared(j + 1);
      const uint32_t b0 = std::max(bit_length(ors[j]), 4u), b1 = next ? bit_length(ors[j + 1]) : 0;
      if (ors[j] && next && ors[j + 1] && b0 + b1 <= MSM_PACK_MAX_BITS &&
          N >= ((size_t)MSM_PACK_MIN_POINTS_PER_BUCKET << (b0 + b1))) {  // (worth it while the points outnumber the buckets)
        uint32_t* packed = c.arena.alloc_n<uint32_t>(N);
        k_pack_u32(c, rts[j], rts[j + 1], b0, N, packed);
        add_job(lay.read_ts(j), packed, true, N);
        jobs.back().known_bits = b0 + b1;
        jobs.back().pack_shift = b0;
        jobs.back().out_second = (G1Affine*)&second[j + 1];
        plan.second_of.push_back(j + 1);
        c.route.v[RouteStats::PACKED_TS]++;
        j++;
      } else {
        add_job(lay.read_ts(j), rts[j], true, N);
        jobs.back().known_bits = bit_length(ors[j]);  // (0 when the counts were not looked at: measured then)
      }
    }
  }
  // E_i = T[dim_j]: commit(E_i) = sum_d T[d] * B_d over the BUCKET sums B_d of dim_j's commitment - no second pass
  // over the N points (msm.hip, MsmJob::derived_parent; falls back to an ordinary column when the window shape of
  // dim_j does not allow it)
  SubtableOrders& orders = *w.tables;
  for (size_t i = 0; i < alpha; i++)
    if (tb.memory_subtable[i] != LH_SUBTABLE_IDENTITY) {
      add_job(lay.E(i), E[i], true, N);
      // (the derived route has no bucket for dim = 0 - msm.hip: T[0] must be 0 - and EQ has T[0] = 1: an ordinary column)
      // A registered subtable asks for the route exactly when its T[0] is 0 (its l is at most 20 by registration).
      bool derive = l <= 20 && tb.memory_subtable[i] != LH_SUBTABLE_EQ;
      if (subtable_is_custom(tb.memory_subtable[i])) {
        uint32_t t0 = 0;
        orders.custom_table(tb.memory_subtable[i], &t0);
        derive = t0 == 0;
      }
      if (derive) {
        MsmJob& jb = jobs.back();
        jb.derived_parent = (int)dim_job[tb.memory_chunk[i]];
        orders.get(tb.memory_subtable[i], &jb.d_table, &jb.d_order);
        jb.table_in_bits = (uint32_t)l, jb.table_out_bits = lasso_subtable_bits(tb.memory_subtable[i], l);
        c.route.v[RouteStats::DERIVED]++;
      }
      jobs.back().known_bits = lasso_subtable_bits(tb.memory_subtable[i], l);  // (l/2)-bit halves combined, or one bit
    }
  // final_cts (2^l entries) is replicated - but an MSM is additive over point ranges (the chunk-then-sum of
  // util/arithmetic/msm.rs:101-114): rank s commits the counts [s 2^l / R, (s + 1) 2^l / R) against the same range of
  // the level's first bases, and the partial commitments join the exchange below - no rank repeats another's additions
  const ReplicatedRange fc_range(sh, M);
  for (size_t j = 0; j < cc; j++) {
    if (shared(j)) continue;
    add_job(lay.final_cts(j), fcs[j] + fc_range.first, true, fc_range.count);
    jobs.back().bases = pcs.commit_bases(nv) + fc_range.first;
    jobs.back().known_bits = bit_length(count_ors[j]);
  }
}
// the batch's results -> the table's commitments, as far as its own jobs made them (what lasso_commit_derive adds, and
// what a table of a batch shares with an earlier one, is still missing)
static std::vector<HG1> lasso_commit_collect(const LassoTable& x, const std::vector<HG1>& part) {
  std::vector<HG1> comms(x.lay.num_polys());
  for (size_t k = 0; k < x.plan.job.size(); k++) comms[x.plan.slot[k]] = part[x.plan.job[k]];
  for (size_t j : x.plan.second_of) comms[x.lay.read_ts(j)] = x.plan.second[j];
  return comms;
}
// the commitments that follow from others by linearity: E_i = dim_j of an identity subtable, a = sum_m coeff_m E_{f(m)}
// under a linear g
static void lasso_commit_derive(const LassoTable& x, std::vector<HG1>& comms) {
  const lh_lasso_table& tb = *x.tb;
  const LassoLayout& lay = x.lay;
  for (size_t i = 0; i < lay.alpha; i++)
    if (tb.memory_subtable[i] == LH_SUBTABLE_IDENTITY) comms[lay.E(i)] = comms[lay.dim(tb.memory_chunk[i])];
  if (!lay.linear_g) return;
  std::vector<host::G1Xyzz> terms(tb.num_terms);
  // (the coefficients of the range / AND / XOR tables are powers of two below 2^64: a few dozen doublings each, done
  // here - waking the host pool for them cost more than they do; wide coefficients go to the pool)
  bool small_coeffs = true;
  for (uint32_t m = 0; m < tb.num_terms && small_coeffs; m++) small_coeffs = lasso_g_coeff_fits(tb, m, 64);
  auto term = [&](size_t m) {
    terms[m] = host::g1_mul(host::g1_from_affine(comms[lay.E(tb.g_factor[m][0])]), lasso_g_coeff(tb, m));
  };
  if (small_coeffs)
    for (size_t m = 0; m < tb.num_terms; m++) term(m);
  else
    host_parallel_for(tb.num_terms, term);
  host::G1Xyzz acc = host::G1Xyzz::identity();
  for (auto& t : terms) acc = host::g1_add(acc, t);
  comms[lay.a()] = host::g1_to_affine(acc);
}

// the output column zero-padded to NV entries (a chunk size above n and no 32-bit form: the table the opening is handed)
static Fr* lasso_pad_a(Ctx& c, const Fr* a, size_t N, size_t NV) {
  Fr* a_pad = c.arena.alloc_n<Fr>(NV);
  LH_HIP(hipMemcpyAsync(a_pad, a, N * sizeof(Fr), hipMemcpyDeviceToDevice, c.stream));
  LH_HIP(hipMemsetAsync(a_pad + N, 0, (NV - N) * sizeof(Fr), c.stream));
  return a_pad;
}
// One table's committed polys as the small-valued columns of the batch opening, its block at small[poly_base]: dim, read_ts
// (below 2^bits of its access counts where known), E, final_cts, and a where it has a 32-bit form - a column of its own under
// a product g (every entry below 2^a_bits), the linear combination x.a_linear of the E columns under a linear g.
// Challenge-free: made as soon as the access counts' widths are known (count_ors).
static void lasso_open_columns(Ctx& c, LassoTable& x, size_t n, size_t poly_base, SmallPoly* small) {
  const lh_lasso_table& tb = *x.tb;
  const LassoLayout& lay = x.lay;
  const Shard sh(c);
  const size_t N = (size_t)1 << (n - sh.rho), M = (size_t)1 << lay.l;
  SmallPoly* s = small + poly_base;
  if (x.a_small && x.w.a_bits) {
    s[lay.a()] = SmallPoly{x.a_small, N, x.w.a_bits};
  } else if (x.a_small) {
    for (uint32_t m = 0; m < tb.num_terms; m++) {
      x.a_linear.poly.push_back(poly_base + lay.E(tb.g_factor[m][0]));
      x.a_linear.coeff.push_back(lasso_g_coeff(tb, m));
    }
    s[lay.a()] = SmallPoly{x.a_small, N, 0, &x.a_linear};
  }
  for (size_t j = 0; j < lay.cc; j++) {
    s[lay.dim(j)] = SmallPoly{x.dims[j], N, (uint32_t)lay.l};
    s[lay.read_ts(j)] = SmallPoly{x.w.rts[j], N, bit_length(x.count_ors[j])};
    s[lay.final_cts(j)] = SmallPoly{x.w.fcs[j], M, 0};
    if (sh.on) {
      // the zero-padded n-variable final_cts column lives in the index range [0, 2^l), l <= shard_bit + rho: this rank's
      // shard of it is the slice [rank * 2^shard_bit, (rank + 1) * 2^shard_bit) at its local indices [0, 2^shard_bit)
      const size_t first = sh.rank << sh.j;
      s[lay.final_cts(j)] = first < M ? SmallPoly{x.w.fcs[j] + first, std::min(M - first, (size_t)1 << sh.j), 0} : SmallPoly{x.w.fcs[j], 0, 0};
    }
  }
  for (size_t i = 0; i < lay.alpha; i++) s[lay.E(i)] = SmallPoly{x.w.E[i], N, lasso_subtable_bits(tb.memory_subtable[i], lay.l)};
}

// The schedule of one table's proof: header, witness, commit, then lasso_argue (r and a(r), Surge, memory check, evaluations)
// and ONE batch opening.  Single-table only: the sharded route, a scheme that commits columns itself, the staged precommit
// (and, inside lasso_argue, ScU32 and the shared quad sums).
void lasso_prove(Ctx& c, const Pcs& pcs, const lh_lasso_table& tb, size_t n, const uint32_t* const* d_dims,
                 Transcript& tr) {
  lasso_check_table(tb);
  LassoTable x(tb, d_dims);
  const LassoLayout& lay = x.lay;
  const size_t cc = lay.cc, l = lay.l, alpha = lay.alpha;
  LH_REQUIRE(n >= 1 && n < 31, LH_ERR_ARG, "lasso: need at least one variable");
  if (n > pcs.max_vars || l > pcs.max_vars)
    throw Error(LH_ERR_INVALID_PCS_PARAM, "Too many variates of poly to commit");
  // every committed poly is zero-padded to nv = max(n, l) variables (spec step 1)
  // Inside a sharded proof (dev.hpp Shard, lh_lasso_prove_sharded) d_dims are this rank's shards of the lookup columns
  // and every n-variable column below is a shard of N = 2^(n - rho) entries; what crosses ranks: the access counters'
  // exchange, partial commitments, partial sums per round, residual tables (sumcheck.cpp, gkr.cpp, mkzg.cpp).  World of one: nothing.
  const Shard sh(c);
  const bool shn = sh.on;
  if (shn) {
    LH_REQUIRE(pcs.shard_bases != nullptr, LH_ERR_ARG, "sharded prove: implemented for multilinear KZG");
    LH_REQUIRE(sh.j >= 1 && l <= sh.j + sh.rho, LH_ERR_ARG,
               "sharded prove: need shard_bit + rho >= chunk_bits (subtables replicated)");
    LH_REQUIRE(sh.sharded(n) && n >= l, LH_ERR_ARG, "sharded prove: 2^num_vars lookups are too few to shard");
  }
  const size_t nv = std::max(n, l), NV = (size_t)1 << (nv - sh.rho);
  const size_t N = (size_t)1 << (n - sh.rho), M = (size_t)1 << l;
  // the committed polys as small-valued columns and the (poly, point) pairs of the batch opening at the end (step 8): r, r_z,
  // r_N, r_M are points 0..3.  Made by the commit batch when the opening's precommit is staged from there, behind the
  // commitments otherwise.  (Ahead of the scope: a precommit on the helper reads them until the scope's end cancels it.)
  std::vector<SmallPoly> small;
  std::vector<lh_evaluation> evs;
  const LassoOpening where = LassoOpening::block(lay);
  auto open_columns = [&] {
    if (!small.empty()) return;
    small.assign(lay.num_polys(), SmallPoly());
    lasso_open_columns(c, x, n, 0, small.data());
    lasso_evaluation_list(lay, where, nullptr, evs);
  };
  LassoPhases phases(c);
  auto lap = [&](int idx) { phases.lap(idx); };

  // ---- witness: counters, subtable reads, lookup outputs
  // (the sorted dim columns only pay off where the MSM sorts slab by slab: msm.hip LH_MSM_SLAB_LOG)
  x.w = lasso_witness_columns(c, tb, n, d_dims, &x.a, &x.a_small, n >= (size_t)knob(Knob::MSM_SLAB_LOG));
  Fr* const a = x.a;
  uint32_t* const a_small = x.a_small;
  const std::vector<uint32_t*>&rts = x.w.rts, &fcs = x.w.fcs, &E = x.w.E;
  lap(0);
  // ---- 0/1: domain separation + commitments (one batched MSM)
  for (size_t v : {n, l, cc, alpha}) tr.common_field_element(HFr::from_u64(v));
  Fr* a_pad = nullptr;  // the output column zero-padded to nv variables, where that table is needed (l > n, no 32-bit form)
  // the opening's column-wise commitments depend on the witness columns alone: on the helper ctx, beside the sum-checks
  // (Options::open_precommit) - in two stages (Options::open_precommit_stages): differences, digits and sort as soon as this
  // commit batch's accumulation is off the chip, the accumulation when the product trees are built
  bool precommit_staged = false;
  if (pcs.commit_columns || pcs.commit_columns_and_write) {
    // a scheme that commits columns itself (Hyrax: vectors of row commitments): a from its 32-bit form when there is one,
    // dim / read_ts / E / final_cts as u32 columns with the bounds known here; E_i of an identity subtable IS dim_j.  The
    // derived, packed and sorted-reuse routes are msm_batch features: their counters stay 0.
    {
      std::vector<const uint32_t*> cols(fcs.begin(), fcs.end());
      k_or_u32(c, cols.data(), cc, M, x.count_ors.data());  // (the access counts bound the timestamps)
    }
    const size_t total = lay.num_polys(), k = pcs.chunks;
    std::vector<PcsColumn> cols(total, PcsColumn{nullptr, true, 0, 1});
    cols[lay.a()] = a_small ? PcsColumn{a_small, true, N, x.w.a_bits ? x.w.a_bits : 32u} : PcsColumn{a, false, N, 0};
    for (size_t j = 0; j < cc; j++) {
      const uint32_t count_bits = std::max(bit_length(x.count_ors[j]), 1u);
      cols[lay.dim(j)] = PcsColumn{d_dims[j], true, N, (uint32_t)l};
      cols[lay.read_ts(j)] = PcsColumn{rts[j], true, N, count_bits};
      cols[lay.final_cts(j)] = PcsColumn{fcs[j], true, M, count_bits};
    }
    for (size_t i = 0; i < alpha; i++)
      if (tb.memory_subtable[i] != LH_SUBTABLE_IDENTITY)
        cols[lay.E(i)] = PcsColumn{E[i], true, N, std::max(lasso_subtable_bits(tb.memory_subtable[i], l), 1u)};
    if (pcs.commit_columns_and_write) {
      // a scheme whose commitments are no points (Brakedown: Merkle roots, and the zero column's is a root like any other,
      // so the identity mask is zero): it writes them itself and finds them again by the columns' pointers at the opening -
      // E_i of an identity subtable under dim_j's, and a without a 32-bit form under the table the opening will be handed
      if (!a_small && N < NV) cols[lay.a()] = PcsColumn{a_pad = lasso_pad_a(c, a, N, NV), false, NV, 0};
      for (size_t i = 0; i < alpha; i++)
        if (tb.memory_subtable[i] == LH_SUBTABLE_IDENTITY) cols[lay.E(i)] = cols[lay.dim(tb.memory_chunk[i])];
      tr.write_field_element(HFr::zero());
      pcs.commit_columns_and_write(cols.data(), total, nv, tr);
    } else {
      std::vector<HG1> comms = pcs.commit_columns(cols.data(), total, nv);
      LH_REQUIRE(comms.size() == total * k, LH_ERR_ARG, "lasso: commit_columns returned the wrong number of points");
      for (size_t i = 0; i < alpha; i++)
        if (tb.memory_subtable[i] == LH_SUBTABLE_IDENTITY) {
          const auto dim = comms.begin() + lay.dim(tb.memory_chunk[i]) * k;
          std::copy(dim, dim + k, comms.begin() + lay.E(i) * k);
        }
      lasso_write_commitments(tr, comms, k);
    }
  } else {
    // zero padding adds nothing to an MSM: commit the unpadded columns against the first entries of the bases.
    // Commitments are linear, so columns that are linear in others need no MSM of their own (same group elements,
    // same proof bytes): E_i = dim_j for an identity subtable, and a = sum_m coeff_m E_{f(m)} when g is linear
    // (range / AND / XOR tables): 4 of 9 column MSMs instead of 9 for the range check.
    // (sharded: this rank's share of the bases; every MSM below is the commitment of a shard - the chunk-split-then-sum
    // of util/arithmetic/msm.rs:101-114 with the shards as chunks - and the partial commitments are added at the end)
    std::vector<MsmJob> jobs;
    lasso_commit_jobs(c, pcs, x, n, nv, false, nullptr, jobs);
    std::vector<HG1>& second = x.plan.second;
    const std::vector<size_t>& second_of = x.plan.second_of;
    std::vector<HG1> part(jobs.size()), comms;
    // (stage 1 of the opening's precommit goes to the helper from behind this batch's accumulation launches; not in a sharded
    // proof, whose commit ends in an exchange, and not under the profiler)
    std::function<void(bool)> stage1 = [&](bool on_aux) {
      open_columns();
      precommit_staged = pcs.precommit(nv, small.data(), small.size(), evs.data(), evs.size(), on_aux ? 1 : 0);
      c.route.v[RouteStats::OPEN_PRECOMMIT_STAGED] = precommit_staged ? 1u : 0u;
    };
    const bool stage = pcs.precommit && c.opt.open_precommit_stages != 0 && !shn && !c.prof;
    msm_batch(c, jobs.data(), jobs.size(), (G1Affine*)part.data(), nullptr, stage ? &stage1 : nullptr);
    c.host_stamp("commit:msm_done");
    if (shn) {
      // partial commitments of the shards (the second outputs of packed jobs included) -> their sums, one exchange
      std::vector<HG1> sums(part);
      for (size_t j : second_of) sums.push_back(second[j]);
      comm_sum_points(c, sums.data(), sums.size());
      for (size_t k = 0; k < part.size(); k++) part[k] = sums[k];
      for (size_t q = 0; q < second_of.size(); q++) second[second_of[q]] = sums[part.size() + q];
    }
    c.host_stamp("commit:summed");
    comms = lasso_commit_collect(x, part);
    lasso_commit_derive(x, comms);
    c.host_stamp("commit:linear");
    lasso_write_commitments(tr, comms);
    c.host_stamp("commit:written");
  }
  lap(1);

  // ---- field-element views only where a sum-check needs tables (E for Surge when g is not linear); dim / read_ts /
  // final_cts (and E under a linear g) stay u32 all the way: fingerprints, evaluations and the batch opening's merge
  // read the 4-byte columns
  std::vector<const Fr*> polys(lay.num_polys(), nullptr);
  open_columns();
  if (a_small) {  // (the output column goes by its 32-bit form: small[a])
  } else if (N < NV) {  // l > n: the output column needs the padding too
    polys[lay.a()] = a_pad ? a_pad : lasso_pad_a(c, a, N, NV);
  } else {
    polys[lay.a()] = a;
  }
  if (!lay.linear_g)  // (under a linear g lasso_argue's Surge sum-check runs over the output column alone)
    for (size_t i = 0; i < alpha; i++) {
      Fr* d = c.arena.alloc_n<Fr>(NV);
      k_fr_from_u32(c, E[i], N, d);
      if (N < NV) LH_HIP(hipMemsetAsync(d + N, 0, (NV - N) * sizeof(Fr), c.stream));
      polys[lay.E(i)] = d;
    }
  const Fr* const* E_fr = polys.data() + lay.E(0);

  // (one stage: all of the precommit starts when the memory-checking argument has built its product trees -
  // prove_grand_product's trees_built: beside the Surge rounds and the tree kernels, which stream at the HBM bound, the
  // helper's sorts only get in the way: tree_up 1.2 -> 5.0 ms per proof.  Two stages: the sorts are through by then, and the
  // callback releases the accumulation)
  std::function<void()> precommit;
  if (pcs.precommit)
    precommit = [&] {
      if (knob(Knob::TEST_PRECOMMIT_GATE) != 0) return;  // (test hook: a prove on which nothing happens at trees_built)
      if (precommit_staged) open_precommit_release(c);
      else pcs.precommit(nv, small.data(), small.size(), evs.data(), evs.size(), -1);
    };

  // ---- 2-7: Surge, memory checking, evaluations
  c.host_stamp("argue:start");
  const LassoClaims cl = lasso_argue(c, tb, n, x.w, d_dims, polys[lay.a()], E_fr, tr, lap, a_small, precommit);
  c.host_stamp("argue:end");

  // ---- 8: ONE batch opening of all committed polys (nv variables) at r, r_z, r_N, r_M (zero-padded)
  std::vector<HFr> points;
  lasso_append_points(points, {&cl.r, &cl.r_z, &cl.r_N, &cl.r_M}, nv);
  lasso_evaluation_values(lay, where, cl, evs.data());
  pcs.batch_open(nv, polys.data(), polys.size(), points.data(), 4, evs.data(), evs.size(), tr, small.data());
  lap(6);
  c.host_stamp("open:end");
  c.host_stamps_print();
  phases.done();
}

// ------------------------------------------------------------------ several tables in one proof (tests/lasso_batch_ref.py)
size_t lasso_batch_check(const lh_lasso_table* const* tables, size_t K, size_t n) {
  LH_REQUIRE(K >= 1 && K <= (size_t)LH_LASSO_BATCH_MAX_TABLES, LH_ERR_ARG,
             "lasso batch: 1 to " + std::to_string(LH_LASSO_BATCH_MAX_TABLES) + " tables");
  LH_REQUIRE(tables != nullptr, LH_ERR_ARG, "null argument: tables");
  LH_REQUIRE(n >= 1 && n < 31, LH_ERR_ARG, "lasso: need at least one variable");
  size_t nv = n, memories = 0, terms = 0, at_n = 0;
  for (size_t t = 0; t < K; t++) {
    LH_REQUIRE(tables[t] != nullptr, LH_ERR_ARG, "null argument: table " + std::to_string(t));
    const lh_lasso_table& tb = *tables[t];
    lasso_check_table(tb);
    const LassoLayout lay(tb);
    // one identity mask (a field element read as 63 bits) frames a table's commitments
    LH_REQUIRE(lay.num_polys() <= 63, LH_ERR_ARG,
               "lasso batch: table " + std::to_string(t) + " has more than 63 commitments (one identity mask per table)");
    nv = std::max<size_t>(nv, tb.chunk_bits);
    memories += lay.alpha, terms += tb.num_terms, at_n += lay.num_at_n();
  }
  // 4 product trees per memory in ONE grand-product GKR, whose layers take 2 B + 1 <= SC_MAX_TABLES tables (gkr.cpp), and the
  // paired leaf layer SC_RW_MAX_PAIRS read / write pairs
  LH_REQUIRE(memories <= (size_t)LASSO_RW_BATCH_MAX && 8 * memories + 1 <= (size_t)SC_MAX_TABLES, LH_ERR_ARG,
             "lasso batch: more than " + std::to_string(LASSO_RW_BATCH_MAX) + " memories in all (4 product trees each in one GKR batch)");
  LH_REQUIRE(terms <= (size_t)LH_SC_MAX_TERMS, LH_ERR_ARG, "lasso batch: too many g terms in all for one Surge sum-check");
  // the batch opening merges every column opened at r_N into one table in one launch (k_lincomb_mixed)
  LH_REQUIRE(at_n <= (size_t)LCM_MAX_SMALL, LH_ERR_ARG, "lasso batch: too many columns opened at one point");
  return nv;
}

void lasso_prove_batch(Ctx& c, const Pcs& pcs, const lh_lasso_table* const* tables, size_t K, size_t n,
                       const uint32_t* const* const* d_dims, Transcript& tr) {
  const size_t nv = lasso_batch_check(tables, K, n);
  LH_REQUIRE(d_dims != nullptr, LH_ERR_ARG, "null argument: d_dims");
  for (size_t t = 0; t < K; t++) {
    LH_REQUIRE(d_dims[t] != nullptr, LH_ERR_ARG, "null argument: d_dims of table " + std::to_string(t));
    for (size_t j = 0; j < tables[t]->num_chunks; j++)
      LH_REQUIRE(d_dims[t][j] != nullptr, LH_ERR_ARG, "null argument: a chunk column of table " + std::to_string(t));
  }
  LH_REQUIRE(!Shard(c).on && !(c.has_comm && c.comm.size > 1), LH_ERR_ARG,
             "lasso batch: sharded batches are not supported (the ctx is inside a sharded prove or has a communicator of several ranks)");
  LH_REQUIRE(pcs.commit_bases && !pcs.commit_columns && !pcs.commit_columns_and_write, LH_ERR_ARG,
             "lasso batch: implemented for schemes that commit columns against bases");
  if (nv > pcs.max_vars) throw Error(LH_ERR_INVALID_PCS_PARAM, "Too many variates of poly to commit");
  const size_t N = (size_t)1 << n, NV = (size_t)1 << nv;
  struct Table : LassoTable {
    using LassoTable::LassoTable;
    std::vector<int> shared_dim_job, shared_table, shared_chunk;  // per chunk: the earlier table's column it shares (-1: none)
    std::vector<HG1> comms;
    size_t poly_base = 0, mem_base = 0;  // of its polys in the opening, of its memories in the batch
  };
  std::vector<Table> T;  // (K entries, reserved: SmallPoly::linear points at a table's a_linear)
  T.reserve(K);
  std::vector<size_t> ls;  // the distinct chunk sizes in order of first appearance: r_M(ls[q]) is point 3 + q
  size_t A = 0, num_polys = 0;
  bool all_linear = true;
  for (size_t t = 0; t < K; t++) {
    T.emplace_back(*tables[t], d_dims[t]);
    Table& x = T.back();
    all_linear = all_linear && x.lay.linear_g;
    x.mem_base = A, x.poly_base = num_polys;
    A += x.lay.alpha, num_polys += x.lay.num_polys();
    if (std::find(ls.begin(), ls.end(), x.lay.l) == ls.end()) ls.push_back(x.lay.l);
  }
  auto point_of_l = [&](size_t l) { return 3 + (size_t)(std::find(ls.begin(), ls.end(), l) - ls.begin()); };
  LassoPhases phases(c);

  // ---- witness, table by table.  A chunk column that an earlier table of the same chunk size was handed too (the same device
  // pointer: AND and XOR over the same operands) is counted once: its read_ts and final_cts serve both tables
  const bool keep_sorted = n >= (size_t)knob(Knob::MSM_SLAB_LOG);
  for (size_t t = 0; t < K; t++) {
    Table& x = T[t];
    const size_t cc = x.lay.cc;
    LassoColumns reuse;
    reuse.rts.assign(cc, nullptr), reuse.fcs.assign(cc, nullptr);
    x.shared_table.assign(cc, -1), x.shared_chunk.assign(cc, -1), x.shared_dim_job.assign(cc, -1);
    for (size_t j = 0; j < cc; j++)
      for (size_t s = 0; s < t && x.shared_table[j] < 0; s++)
        for (size_t k = 0; k < T[s].lay.cc && T[s].lay.l == x.lay.l; k++)
          if (T[s].dims[k] == x.dims[j] && T[s].shared_table[k] < 0) {  // (the table that counted it)
            x.shared_table[j] = (int)s, x.shared_chunk[j] = (int)k;
            reuse.rts[j] = T[s].w.rts[k], reuse.fcs[j] = T[s].w.fcs[k];
            break;
          }
    x.w = lasso_witness_columns(c, *x.tb, n, x.dims, &x.a, &x.a_small, keep_sorted, &reuse);
  }
  phases.lap(0);

  // ---- 0/1: domain separation, then every table's commitments from ONE batched MSM
  tr.common_field_element(HFr::from_u64(K));
  tr.common_field_element(HFr::from_u64(n));
  for (const Table& x : T)
    for (size_t v : {x.lay.l, x.lay.cc, x.lay.alpha}) tr.common_field_element(HFr::from_u64(v));
  {
    // the access counts' widths (they bound the timestamps: packing, known_bits): one readback per distinct chunk size
    if (c.opt.lasso_pack_ts != 0 && N >= ((size_t)1 << 12))
      for (size_t l : ls) {
        std::vector<const uint32_t*> cols;
        for (const Table& x : T)
          if (x.lay.l == l) cols.insert(cols.end(), x.w.fcs.begin(), x.w.fcs.end());
        std::vector<uint32_t> ors(cols.size(), 0);
        k_or_u32(c, cols.data(), cols.size(), (size_t)1 << l, ors.data());
        size_t at = 0;
        for (Table& x : T)
          if (x.lay.l == l)
            for (uint32_t& o : x.count_ors) o = ors[at++];
      }
    std::vector<MsmJob> jobs;
    for (Table& x : T) {
      for (size_t j = 0; j < x.lay.cc; j++)
        if (x.shared_table[j] >= 0) x.shared_dim_job[j] = (int)T[x.shared_table[j]].plan.dim_job[x.shared_chunk[j]];
      lasso_commit_jobs(c, pcs, x, n, nv, true, x.shared_dim_job.data(), jobs);
    }
    std::vector<HG1> part(jobs.size());
    msm_batch(c, jobs.data(), jobs.size(), (G1Affine*)part.data());
    for (Table& x : T) {
      x.comms = lasso_commit_collect(x, part);
      for (size_t j = 0; j < x.lay.cc; j++)
        if (x.shared_table[j] >= 0) {
          const Table& s = T[x.shared_table[j]];
          const size_t k = (size_t)x.shared_chunk[j];
          x.comms[x.lay.dim(j)] = s.comms[s.lay.dim(k)];
          x.comms[x.lay.read_ts(j)] = s.comms[s.lay.read_ts(k)];
          x.comms[x.lay.final_cts(j)] = s.comms[s.lay.final_cts(k)];
        }
      lasso_commit_derive(x, x.comms);
      lasso_write_commitments(tr, x.comms);
    }
  }
  phases.lap(1);

  // ---- 2: r, and a_t(r) for every table
  const std::vector<HFr> r = tr.squeeze_challenges(n);
  {
    std::vector<const uint32_t*> cols;
    std::vector<const Fr*> frs;
    for (const Table& x : T) {
      if (x.a_small) cols.push_back(x.a_small);
      else frs.push_back(x.a);
    }
    std::vector<HFr> vs(cols.size()), vf;
    if (!cols.empty()) lasso_evaluate_u32(c, cols.data(), cols.size(), r.data(), n, false, vs.data());
    if (!frs.empty()) vf = evaluate_polys(c, frs.data(), frs.size(), n, r.data(), false);
    size_t is = 0, ifr = 0;
    for (Table& x : T) x.cl.v = x.a_small ? vs[is++] : vf[ifr++];
  }
  for (const Table& x : T) tr.write_field_element(x.cl.v);

  // ---- 3: ONE Surge sum-check over eq * sum_t rho^t g_t
  const HFr rho = tr.squeeze_challenge();
  std::vector<HFr> rho_pow(K, HFr::one());
  for (size_t t = 1; t < K; t++) rho_pow[t] = rho_pow[t - 1] * rho;
  HFr claim = HFr::zero();
  for (size_t t = 0; t < K; t++) claim += rho_pow[t] * T[t].cl.v;
  std::vector<HFr> r_z, e_rz;
  ScOptions so;
  so.sum_is_exact = true;
  if (all_linear) {
    // every g linear: the summand is eq * sum_t rho^t a_t entry by entry - ONE table, as in lasso_argue's linear case -
    // formed from the output columns; the evaluations E_t,i(r_z) are inner products of the 32-bit columns with eq(r_z)
    {
      ArenaScope inner(c.arena);
      Fr* comb = c.arena.alloc_n<Fr>(N);
      std::vector<const Fr*> frs;
      std::vector<Fr> wfr, wsm;
      std::vector<const uint32_t*> sm;
      std::vector<size_t> sm_len;
      for (size_t t = 0; t < K; t++) {
        if (T[t].a_small) sm.push_back(T[t].a_small), sm_len.push_back(N), wsm.push_back(dev(rho_pow[t]));
        else frs.push_back(T[t].a), wfr.push_back(dev(rho_pow[t]));
      }
      k_lincomb_mixed(c, frs.data(), wfr.data(), frs.size(), sm.data(), sm_len.data(), wsm.data(), sm.size(), N, comb);
      const Fr* tab = comb;
      r_z = sum_check_prove(c, LH_SC_EVALUATIONS, n, lasso_one_term(), &tab, 1, r.data(), 1, claim, tr, so).challenges;
    }
    std::vector<const uint32_t*> cols;
    for (const Table& x : T) cols.insert(cols.end(), x.w.E.begin(), x.w.E.end());
    e_rz.assign(A, HFr::zero());  // (the table of r_z[1..] stays for the batch opening at r_z)
    lasso_evaluate_u32(c, cols.data(), A, r_z.data(), n, false, e_rz.data());
  } else {
    // one expression with every table's terms, table t's scaled by rho^t, over the field-element views of all E columns
    std::vector<const Fr*> E_fr(A, nullptr);
    lh_sop surge;
    memset(&surge, 0, sizeof(surge));
    for (size_t t = 0; t < K; t++) {
      const Table& x = T[t];
      for (size_t i = 0; i < x.lay.alpha; i++) {
        Fr* d = c.arena.alloc_n<Fr>(N);
        k_fr_from_u32(c, x.w.E[i], N, d);
        E_fr[x.mem_base + i] = d;
      }
      lasso_append_g(surge, *x.tb, x.mem_base, &rho_pow[t]);
    }
    SumCheckResult sc = sum_check_prove(c, LH_SC_EVALUATIONS, n, surge, E_fr.data(), A, r.data(), 1, claim, tr, so);
    r_z = sc.challenges, e_rz = sc.evals;
  }
  tr.write_field_elements(e_rz);
  for (Table& x : T) x.cl.e_rz.assign(e_rz.begin() + x.mem_base, e_rz.begin() + x.mem_base + x.lay.alpha);
  phases.lap(2);

  // ---- 4: memory checking, ONE grand-product GKR: the n-variable trees RS, WS of every memory, then Init, Final of every memory
  const HFr gamma = tr.squeeze_challenge(), tau = tr.squeeze_challenge(), gamma2 = gamma * gamma;
  std::vector<HFr> r_N;
  std::vector<std::vector<HFr>> r_M(ls.size());
  {
    ArenaScope inner(c.arena);
    MemoryTrees trees(A, n);
    // (lasso_argue: the level above the leaves comes with them from 2^12 lookups on, and the write leaves are not stored
    // where n is above every chunk size)
    const size_t max_l = *std::max_element(ls.begin(), ls.end());
    const bool fused_up = n >= GP_LEVEL_UP_MIN_VARS, ws_implicit = fused_up && n > max_l;
    LassoRwBatch rw;
    memset(&rw, 0, sizeof(rw));
    for (const Table& x : T)
      for (size_t i = 0; i < x.lay.alpha; i++) {
        const size_t b = x.mem_base + i, j = x.tb->memory_chunk[i];
        const MemoryTrees::Memory m = trees.add(c, b, N, x.lay.l, fused_up, ws_implicit);
        rw.dim[b] = x.dims[j], rw.e[b] = x.w.E[i], rw.ts[b] = x.w.rts[j];
        rw.rs[b] = m.rs, rw.ws[b] = m.ws, rw.rs_up[b] = m.rs_up, rw.ws_up[b] = m.ws_up;
        k_lasso_if_leaves(c, (int)x.tb->memory_subtable[i], (uint32_t)x.lay.l, x.w.fcs[j], (size_t)1 << x.lay.l, dev(gamma),
                          dev(gamma2), dev(tau), m.init, m.fin, x.w.T.empty() ? nullptr : x.w.T[i]);
      }
    k_lasso_rw_leaves_batch(c, rw, A, N, fused_up, dev(gamma), dev(gamma2), dev(tau));
    phases.lap(3);
    GrandProductResult gp = trees.prove(c, tr);
    r_N = gp.points[0];
    for (const Table& x : T) r_M[point_of_l(x.lay.l) - 3] = gp.points[2 * A + 2 * x.mem_base];
  }
  phases.lap(4);

  // ---- 5: evaluations at r_N (dim | read_ts | E of every table, one pass) and at r_M(l) (final_cts, per chunk size)
  {
    std::vector<const uint32_t*> at_n;
    for (const Table& x : T) {
      at_n.insert(at_n.end(), x.dims, x.dims + x.lay.cc);
      at_n.insert(at_n.end(), x.w.rts.begin(), x.w.rts.end());
      at_n.insert(at_n.end(), x.w.E.begin(), x.w.E.end());
    }
    std::vector<HFr> ev_n(at_n.size());
    lasso_evaluate_u32(c, at_n.data(), at_n.size(), r_N.data(), n, false, ev_n.data());
    size_t at = 0;
    for (Table& x : T) {
      x.cl.ev_n.assign(ev_n.begin() + at, ev_n.begin() + at + x.lay.num_at_n());
      at += x.lay.num_at_n();
    }
    for (size_t q = 0; q < ls.size(); q++) {
      std::vector<const uint32_t*> at_l;
      for (const Table& x : T)
        if (x.lay.l == ls[q]) at_l.insert(at_l.end(), x.w.fcs.begin(), x.w.fcs.end());
      std::vector<HFr> ev_l(at_l.size());
      evaluate_u32_columns(c, at_l.data(), at_l.size(), r_M[q].data(), ls[q], ev_l.data());
      size_t k = 0;
      for (Table& x : T)
        if (x.lay.l == ls[q]) x.cl.ev_l.assign(ev_l.begin() + k, ev_l.begin() + k + x.lay.cc), k += x.lay.cc;
    }
  }
  for (const Table& x : T) tr.write_field_elements(x.cl.ev_n), tr.write_field_elements(x.cl.ev_l);
  phases.lap(5);

  // ---- 6: ONE batch opening over nv variables: polys table-major, points r, r_z, r_N, r_M per chunk size (zero-padded)
  // (the opening's precommit on the helper ctx is not started on this path: DESIGN.md §17)
  {
    std::vector<SmallPoly> small(num_polys, SmallPoly());
    std::vector<const Fr*> polys(num_polys, nullptr);
    std::vector<lh_evaluation> evs;
    for (Table& x : T) {
      lasso_open_columns(c, x, n, x.poly_base, small.data());
      // (no 32-bit form: the field-element table - padded where a chunk size is above n)
      if (!x.a_small) polys[x.poly_base + x.lay.a()] = N < NV ? lasso_pad_a(c, x.a, N, NV) : x.a;
      lasso_evaluation_list(x.lay, LassoOpening::block(x.lay, x.poly_base, point_of_l(x.lay.l)), &x.cl, evs);
    }
    std::vector<const std::vector<HFr>*> pts = {&r, &r_z, &r_N};
    for (const std::vector<HFr>& pt : r_M) pts.push_back(&pt);
    std::vector<HFr> points;
    lasso_append_points(points, pts, nv);
    pcs.batch_open(nv, polys.data(), num_polys, points.data(), pts.size(), evs.data(), evs.size(), tr, small.data());
  }
  phases.lap(6);
  phases.done();
}

}  // namespace lh
