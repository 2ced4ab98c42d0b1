// Caller-registered Lasso subtables (include/lasso_hip.h lh_subtable_register): host only, no ctx - the verifier has none.
// A registered table is immutable and reference-counted: whoever looked it up (a prove, a verify) keeps it alive while
// another thread unregisters it.  Kinds come from a counter that only goes up, so a stale kind is never another table.
#include <memory>
#include "host.hpp"

namespace lh {

namespace {
std::mutex g_mu;
std::map<uint32_t, std::shared_ptr<const CustomSubtable>> g_tables;
uint32_t g_next = 0;  // registrations so far in this process
}  // namespace

uint32_t subtable_register(const uint32_t* values, uint32_t chunk_bits) {
  LH_REQUIRE(values != nullptr, LH_ERR_ARG, "null argument: values");
  LH_REQUIRE(chunk_bits >= 1 && chunk_bits <= LH_SUBTABLE_CUSTOM_MAX_BITS, LH_ERR_ARG,
             "subtable: chunk_bits must be in [1, LH_SUBTABLE_CUSTOM_MAX_BITS]");
  auto t = std::make_shared<CustomSubtable>();
  const size_t M = (size_t)1 << chunk_bits;
  t->chunk_bits = chunk_bits;
  t->values.assign(values, values + M);
  uint32_t all = 0;
  for (uint32_t v : t->values) all |= v;
  t->value_bits = all ? 32u - (uint32_t)__builtin_clz(all) : 0u;
  if (t->values[0] == 0) {
    // the indices sorted by entry, for the derived commitments (MsmJob::d_order; asked for exactly when T[0] = 0): made once
    // here, not per prove.  32-bit values: a counting sort would want 2^32 counters, so a stable LSD radix sort by 16-bit
    // digits, one pass per digit the entries have.
    std::vector<uint32_t> cur(M), next(M);
    for (size_t d = 0; d < M; d++) cur[d] = (uint32_t)d;
    for (uint32_t shift = 0; shift < t->value_bits; shift += 16) {
      std::vector<uint32_t> start((size_t)1 << 16 | 1, 0);
      for (size_t d = 0; d < M; d++) start[((t->values[d] >> shift) & 0xffffu) + 1]++;
      for (size_t v = 0; v < ((size_t)1 << 16); v++) start[v + 1] += start[v];
      for (size_t p = 0; p < M; p++) next[start[(t->values[cur[p]] >> shift) & 0xffffu]++] = cur[p];
      cur.swap(next);
    }
    t->order = std::move(cur);
  }
  Keccak256 k;  // of the values as little-endian 32-bit words
  std::vector<uint8_t> le(4 * M);
  for (size_t i = 0; i < M; i++)
    for (int b = 0; b < 4; b++) le[4 * i + b] = (uint8_t)(t->values[i] >> (8 * b));
  k.update(le.data(), le.size());
  k.finalize_reset(t->digest);
  std::lock_guard<std::mutex> lock(g_mu);
  LH_REQUIRE(g_tables.size() < (size_t)LH_SUBTABLE_CUSTOM_MAX, LH_ERR_ARG,
             "subtable: LH_SUBTABLE_CUSTOM_MAX subtables are registered already");
  LH_REQUIRE(g_next < 0xffffffffu - LH_SUBTABLE_CUSTOM_BASE, LH_ERR_ARG, "subtable: out of kinds");
  t->kind = LH_SUBTABLE_CUSTOM_BASE + g_next++;
  g_tables[t->kind] = t;
  return t->kind;
}

void subtable_unregister(uint32_t kind) {
  std::lock_guard<std::mutex> lock(g_mu);
  LH_REQUIRE(g_tables.erase(kind) == 1, LH_ERR_ARG, "subtable: not a registered kind");
}

std::shared_ptr<const CustomSubtable> subtable_find(uint32_t kind) {
  std::lock_guard<std::mutex> lock(g_mu);
  auto it = g_tables.find(kind);
  return it == g_tables.end() ? nullptr : it->second;
}

std::shared_ptr<const CustomSubtable> subtable_require(uint32_t kind, size_t l) {
  std::shared_ptr<const CustomSubtable> t = subtable_find(kind);
  LH_REQUIRE(t != nullptr, LH_ERR_ARG, "lasso: subtable kind is not registered");
  LH_REQUIRE(t->chunk_bits == l, LH_ERR_ARG, "lasso: chunk_bits differs from the registered subtable's");
  return t;
}

}  // namespace lh
