// The steps the arguments share (host.hpp "steps shared by the arguments"): refusals, the commitment and evaluation of
// u32 columns, the memory-checking trees, the verifiers' table fold and verdict.  Lasso, LogUp-GKR, memory checking and
// Spark are written from these.
#include <algorithm>
#include "host.hpp"

namespace lh {

void argument_not_sharded(Ctx& c, const std::string& name) {
  LH_REQUIRE(!Shard(c).on && !(c.has_comm && c.comm.size > 1), LH_ERR_ARG,
             name + ": sharded proofs are not supported (the ctx is inside a sharded prove or has a communicator of several ranks)");
}
void argument_pcs_check(const Pcs& pcs, size_t nv, const std::string& name, bool needs_batch_commit) {
  LH_REQUIRE(pcs.chunks == 1 && (!needs_batch_commit || pcs.batch_commit) && pcs.commit_bases && !pcs.commit_and_write &&
                 !pcs.commit_columns_and_write,
             LH_ERR_ARG, name + ": implemented for schemes whose commitment is one point over bases");
  if (nv > pcs.max_vars) throw Error(LH_ERR_INVALID_PCS_PARAM, "Too many variates of poly to commit");
}
void argument_pcs_check(const PcsVerifier& pcs, const std::string& name) {
  LH_REQUIRE(pcs.chunks == 1 && !pcs.read_commitments, LH_ERR_ARG, name + ": implemented for commitments of one point");
}

std::vector<HG1> commit_u32_columns(Ctx& c, const Pcs& pcs, size_t nv, const std::vector<U32Column>& cols, uint32_t* bits) {
  std::vector<uint32_t> ors(cols.size(), 0);
  std::vector<char> have(cols.size(), 0);
  for (size_t k = 0; k < cols.size(); k++)
    if (cols[k].known_or) ors[k] = *cols[k].known_or, have[k] = 1;
  for (size_t k = 0; k < cols.size(); k++) {  // the columns of cols[k]'s length that are still without their OR
    if (have[k]) continue;
    std::vector<size_t> at;
    std::vector<const uint32_t*> ptrs;
    for (size_t i = k; i < cols.size(); i++)
      if (!have[i] && cols[i].len == cols[k].len) at.push_back(i), ptrs.push_back(cols[i].ptr), have[i] = 1;
    std::vector<uint32_t> o(at.size(), 0);
    k_or_u32(c, ptrs.data(), ptrs.size(), cols[k].len, o.data());
    for (size_t t = 0; t < at.size(); t++) ors[at[t]] = o[t];
  }
  std::vector<MsmJob> jobs;
  for (size_t k = 0; k < cols.size(); k++) {
    bits[k] = std::max(bit_length(ors[k]), 1u);
    jobs.push_back(MsmJob{cols[k].ptr, true, pcs.commit_bases(nv), cols[k].len});
    jobs.back().known_bits = bits[k];
  }
  std::vector<HG1> comms(jobs.size());
  msm_batch(c, jobs.data(), jobs.size(), (G1Affine*)comms.data());
  return comms;
}

void evaluate_u32_columns(Ctx& c, const uint32_t* const* cols, size_t count, const HFr* point, size_t vars, HFr* out) {
  ArenaScope scope(c.arena);
  const size_t len = (size_t)1 << vars;
  Fr* eq = c.arena.alloc_n<Fr>(len);
  k_eq_xy(c, (const Fr*)point, vars, eq);
  k_inner_products_small(c, cols, count, eq, len, (Fr*)out);
}

MemoryTrees::Memory MemoryTrees::add(Ctx& c, size_t b, size_t N, size_t l, bool up_n, bool ws_implicit, bool up_l) {
  const size_t M = (size_t)1 << l;
  Memory m{};
  m.rs = c.arena.alloc_n<Fr>(N);
  m.ws = ws_implicit ? nullptr : c.arena.alloc_n<Fr>(N);
  if (up_n) m.rs_up = c.arena.alloc_n<Fr>(N / 2), m.ws_up = c.arena.alloc_n<Fr>(N / 2);
  m.init = c.arena.alloc_n<Fr>(M), m.fin = c.arena.alloc_n<Fr>(M);
  if (up_l) m.init_up = c.arena.alloc_n<Fr>(M / 2), m.fin_up = c.arena.alloc_n<Fr>(M / 2);
  leaves[2 * b] = m.rs, leaves[2 * b + 1] = m.ws;
  level_up[2 * b] = m.rs_up, level_up[2 * b + 1] = m.ws_up;
  plus_one[2 * b + 1] = 1;
  leaves[2 * A + 2 * b] = m.init, leaves[2 * A + 2 * b + 1] = m.fin;
  level_up[2 * A + 2 * b] = m.init_up, level_up[2 * A + 2 * b + 1] = m.fin_up;
  depths[2 * A + 2 * b] = depths[2 * A + 2 * b + 1] = l;
  return m;
}

HFr host_table_eval(size_t l, const std::vector<HFr>& x, const std::function<HFr(size_t)>& row) {
  std::vector<HFr> cur(((size_t)1 << l) / 2);
  const size_t chunks = std::min<size_t>(cur.size(), 64);  // (the pool hands out items one by one)
  host_parallel_for(chunks, [&](size_t ch) {
    for (size_t k = ch * cur.size() / chunks; k < (ch + 1) * cur.size() / chunks; k++) {
      const HFr lo = row(2 * k), hi = row(2 * k + 1);
      cur[k] = lo + x[0] * (hi - lo);
    }
  });
  for (size_t i = 1; i < l; i++) {
    const size_t half = cur.size() / 2;
    for (size_t k = 0; k < half; k++) cur[k] = cur[2 * k] + x[i] * (cur[2 * k + 1] - cur[2 * k]);
    cur.resize(half);
  }
  return cur[0];
}

void argument_verdict(const std::string& name, const std::function<void()>& verify) {
  try {
    verify();
  } catch (const Error& e) {
    if (e.code == LH_ERR_INVALID_SUMCHECK || e.code == LH_ERR_INVALID_PCS_OPEN || e.code == LH_ERR_TRANSCRIPT ||
        e.code == LH_ERR_SERIALIZATION)
      throw Error(LH_ERR_INVALID_SNARK, name + ": " + e.msg);
    throw;
  }
}

void argument_absorb_commitments(Transcript& tr, const std::vector<HG1>& comms) {
  uint64_t mask = 0;
  for (size_t i = 0; i < comms.size(); i++)
    if (comms[i].is_identity()) mask |= (uint64_t)1 << i;
  tr.common_field_element(HFr::from_u64(mask));
  for (const HG1& cm : comms)
    if (!cm.is_identity()) tr.common_commitment(cm);
}

std::vector<HG1> argument_read_commitment_blob(const std::string& name, const uint8_t* blob, size_t len, size_t count) {
  KeccakTranscript kt;
  kt.stream.assign(blob, blob + len);
  Transcript tr(&kt.vt);
  std::vector<HG1> comms;
  try {
    comms = lasso_read_commitments(tr, count);
  } catch (const Error& e) {
    throw Error(LH_ERR_INVALID_SNARK, name + ": malformed commitment: " + e.msg);
  }
  if (kt.pos != kt.stream.size()) throw Error(LH_ERR_INVALID_SNARK, name + ": malformed commitment: wrong length");
  return comms;
}

}  // namespace lh
