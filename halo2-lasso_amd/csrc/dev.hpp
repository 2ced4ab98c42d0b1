// Internal: device context, workspace arena, kernel launcher declarations.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdarg.h>
#include <stdio.h>
#include <functional>
#include <memory>
#include <string>
#include <vector>
#include <utility>
#include <stdexcept>

#include "../../include/lasso_hip.h"
#include "ec.cuh"
#include "round.cuh"  // ScFinishArgs, SC_LANE_TAG_SHIFT

namespace lh {

// ------------------------------------------------------------------ errors
struct Error : std::exception {
  int code;
  std::string msg;
  Error(int c, std::string m) : code(c), msg(std::move(m)) {}
  const char* what() const noexcept override { return msg.c_str(); }
};

void set_last_error(const char* msg);

#define LH_HIP(expr)                                                                       \
  do {                                                                                     \
    hipError_t e_ = (expr);                                                                \
    if (e_ != hipSuccess)                                                                  \
      throw ::lh::Error(LH_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

#define LH_REQUIRE(cond, code, text) \
  do {                               \
    if (!(cond)) throw ::lh::Error((code), (text)); \
  } while (0)

}  // namespace lh
#include "owned.hpp"
namespace lh {

// ------------------------------------------------------------------ workspace arena
// Stack-disciplined device allocator: the prover's temporaries nest (per sum-check, per layer),
// so a bump pointer with mark/release avoids hipMalloc/hipFree (both synchronise) on the hot path.
class Arena {
 public:
  struct Mark {
    size_t block, used;
  };
  void* alloc(size_t bytes);
  void* alloc_raw(size_t bytes);
  template <class T>
  T* alloc_n(size_t n) {
    return (T*)alloc(n * sizeof(T));
  }
  Mark mark() const { return {cur_, blocks_.empty() ? 0 : blocks_[cur_].used}; }
  void release(Mark m);
  size_t high_water() const { return high_; }
  size_t reserved() const {  // bytes held from the device
    size_t t = 0;
    for (const Block& b : blocks_) t += b.size;
    return t;
  }

 private:
  struct Block {
    DevMem mem;
    size_t size, used;
  };
  std::vector<Block> blocks_;
  size_t cur_ = 0, high_ = 0;
};

struct ArenaScope {
  Arena& a;
  Arena::Mark m;
  explicit ArenaScope(Arena& a_) : a(a_), m(a_.mark()) {}
  ~ArenaScope() { a.release(m); }
};

// ------------------------------------------------------------------ per-kernel profiling (off by default)
// When enabled every instrumented launch is bracketed by HIP events on the ctx stream and synchronised,
// so the per-kernel durations are exact but the prove as a whole is slower: bench.py runs its timed
// region with profiling off and a separate profiled pass for the roofline numbers.
struct ProfRec {
  char name[40];
  double ms;     // HIP-event duration
  double bytes;  // algorithmic bytes of the launch (SURVEY.md §8d formulas)
  double muls;   // field multiplications of the launch (integer-ALU roofline)
  double items;  // work items (pairs, points, ...)
};

constexpr uint32_t FIN_LANE_SUMS = 65536;  // partial sums the lane buffer holds (a launch's workgroups x its sums per workgroup)

// ------------------------------------------------------------------ route options and the route a proof took
// The switches that decide WHICH code proves (not how fast a kernel runs).  Per ctx: set through lh_ctx_set_option
// (include/lasso_hip.h lists them), initialised at ctx creation from the environment variable of the same name in upper
// case with an LH_ prefix (LH_OPEN_SMALL_MIN_VARS, ...).  Proof bytes never depend on them.
struct Options {
  int64_t open_small_min_vars = 21;    // smallest opening whose largest quotient(s) are committed column by column (64: never)
  bool open_small_min_vars_forced = false;  // set explicitly: no automatic "few columns" exception below the threshold
  int64_t open_small_depth = 0;        // 1 / 2: that many column-wise quotient levels whatever the shape (0: by cost)
  int64_t sc_eq_factoring = 1;         // 0: every sum-check round streams and binds its eq tables
  int64_t lasso_pack_ts = 1;           // 0: one MSM pass per read_ts column
  int64_t sc_tail = 1;                 // 0: one launch per sum-check round all the way down (no resident tail)
  int64_t sc_tail_max_len = 8192;      // longest table that enters the resident tail
  int64_t shard_exchange_log = 19;     // sharded sum-check: the residual tables travel once they hold <= 2^this entries
                                       // (17 until round 5; 19 removes two sharded rounds - two collectives - per sum-check at
                                       // the same per-rank compute time, 20 two more for +2 % of it: tools/r05_xlog_sweep.sh)
  int64_t open_precommit = 1;          // proofs of >= 2^this lookups run the challenge-free half of the opening's column route
                                       // (the MSMs over differences of witness columns) on a helper ctx beside the sum-checks of
                                       // a Lasso prove (0: never; 1: always)
  int64_t open_precommit_stages = 1;   // 1: that precommit runs in two stages - column differences, digits and sort (memory-bound)
                                       // as soon as the commit batch's bucket accumulation has left the chip, the bucket
                                       // accumulation (ALU-bound) when the product trees are built; 0: all of
                                       // it when the trees are built.  Sharded proofs and profiled proves: one stage
  int64_t msm_window_tables = 0;       // SRS levels of <= 2^this points get a window table (MsmJob::win_table) on first use:
                                       // full-width columns over them reduce ONE bucket set (0: no tables)
  int64_t sc_pp_fold = 1;              // 0: the generic layers of the grand products keep their coefficients as products of
                                       // every round (sc_round_e2) instead of folding them into the left factors and sharing
                                       // Montgomery reductions (sc_round_pp); the leaf layers (ScRwRound) keep cs and k
                                       // outside their tables and run the leaf kernel in every streaming round
                                       // 2: sc_round_pp in every streaming round, nothing folded (coefficients applied on the way)
  int64_t msm_half_batches = 1;        // an MSM batch of >= 2^24 entries runs as two halves: the first half's latency-bound tails
                                       // (continuation levels, bucket reduction, window sums) on the aux stream beside the
                                       // second half's accumulation (msm.hip msm_pick_split; 0: one batch, one stream)
  int64_t gkr_resident = 1;            // the layers of a grand-product argument whose tables fit the resident kernel run in ONE
                                       // launch (layer loop, eq tables and rounds inside; 0: one sum-check per layer)
  int64_t comm_round = 0;              // how the partial sums of a sharded sum-check round are combined: 0 = all-gather +
                                       // a sum-and-publish kernel; 1 = ONE collective, ncclAllReduce(ncclSum) over u64 lanes
                                       // of 32-bit limbs straight into the pinned memory the host polls (lazy reduction mod
                                       // r on the host, no kernel behind the collective); 2 = the same all-reduce into
                                       // device memory followed by a copy to the host (should a fabric refuse host memory
                                       // as a receive buffer).  Same proof bytes; unmeasured on more than one GPU.
  int64_t hyrax_rows = 1;              // Hyrax commits every row of every poly with the row kernels (kernels_hyrax.hip: one bucket
                                       // set per row over the generators' window table, no host wait between rows); 0: one
                                       // msm_batch job per row
  int64_t brakedown_batch_commit = 1;  // lh_brakedown_batch_commit runs its polys as one batch (brakedown.cpp); 0: a commit each
  int64_t brakedown_staged_open = 0;   // lh_brakedown_batch_open reads the opened columns from the matrix staged on the host
  int64_t brakedown_u32_gather = 1;    // a column commit runs the first encoder stage of its u32 columns from the 4-byte
                                       // entries (kernels_brakedown.hip bd_gather_u32); 0: bd_gather on the loaded message
  int64_t logup_fused_leaves = 1;      // LogUp-GKR (logup.cpp): the leaves of a side's fractions and the level above them in
                                       // ONE launch (kernels_logup.hip logup_leaves_up); 0: the leaves, then one frac_up each
  Options();                           // environment defaults (dev.cpp)
  int64_t* find(const char* name);
  static bool in_range(const char* name, int64_t value);  // the range lh_ctx_set_option accepts
};

// ------------------------------------------------------------------ process-wide knobs
// Every other LH_* variable the library reads: one row each in KNOB_TABLE (dev.cpp: name, kind, default, accepted range),
// parsed like the options' defaults (unset or empty: the default; unparsable or out of range: the default and one line on
// stderr).  Read on first use and kept for the process, except the rows the table marks live (read at every use).
enum class Knob {  // (grouped as the table: thresholds, A/B switches, operation, diagnostics, test hooks)
  SC_TAIL_G, MSM_C_OFF, MSM_C_MAX, MSM_K2, MSM_SEG, MSM_SLAB_LOG, MSM_TREE_MAX, MSM_QUAD_MAX, MSM_TWO_LEVEL, MSM_HALF_MIN_LOG,
  MSM_HALF_COVER, EXPR_MONOMIALS, EXPR_JIT_MIN_VARS, EXPR_EF_MIN_VARS,
  FIN_LANES_MIN_BYTES, SC_U32, OPEN_U32_ROUNDS, OPEN_FOLD_COLS, OPEN_SHARE_SUMS, LASSO_PRODUCT_U32,
  HOST_THREADS, JIT_CACHE, JIT_CACHE_DIR, EXPR_JIT, SC_TAIL_TIMEOUT_MS, GKR_START_TIMEOUT_MS, COMM_WAIT_TIMEOUT_MS, COMM_A2A,
  COMM_PROBE,
  HOST_TRACE, SC_TAIL_TRACE, GKR_TRACE, SC_DEBUG, MSM_DEBUG, HP_DEBUG, COMM_DEBUG, OPEN_SMALL_CHECK,
  COMM_A2A_SELF, COMM_PROBE_FAIL, SHARDED_COUNTERS_MIN_R, TEST_PRECOMMIT_GATE,
  COUNT
};
double knob(Knob k);            // the value (switches 0 / 1; LH_COMM_A2A: 1 = allgather)
const char* knob_text(Knob k);  // a path knob's value (nullptr: unset or empty)
struct RouteStats {  // lh_lasso_route (include/lasso_hip.h): counters of the last Lasso prove on the ctx
  uint32_t v[LH_LASSO_ROUTE_WORDS] = {0};
  enum { OPEN_DEPTH, OPEN_PASSES, EF_ROUNDS, STD_ROUNDS, RW_ROUNDS, TAILS, TAIL_ROUNDS, PACKED_TS, DERIVED, SORTED_REUSE,
         SHARDED_ROUNDS, SHARD_EXCHANGES, WIN_TABLE_JOBS, OPEN_PRECOMMIT, RESIDENT_LAYERS, PP_FOLDS, MSM_HALF_BATCHES,
         OPEN_SHARED_SUMS, OPEN_PRECOMMIT_STAGED };
};

// ------------------------------------------------------------------ a long-lived host thread (dev.cpp)
// Runs submitted tasks one after the other: the driver of a helper ctx (open_columns.cpp open_precommit_*) - starting a
// std::thread per proof costs tens of microseconds on the prover's critical path, a condition variable costs two.
class HostWorker {
 public:
  HostWorker();
  ~HostWorker();  // finishes what was submitted, then joins
  void submit(std::function<void()> fn);
  void wait();    // until every submitted task has finished
 private:
  struct Impl;
  Impl* impl_;
};

// ------------------------------------------------------------------ context
struct OpenPrecommit;  // open_columns.hpp
struct Ctx {
  Options opt;
  RouteStats route;
  int device = 0;
  Ctx() = default;  // options and knobs only, no device behind it (lh_debug_msm_plan)
  // on `device_id`, which it leaves current; throws LH_ERR_DEVICE (what was created by then goes with the members)
  explicit Ctx(int device_id);
  ~Ctx();  // the ordered part of the teardown (dev.cpp); the members release themselves
  Ctx(const Ctx&) = delete;
  Ctx& operator=(const Ctx&) = delete;
  Stream stream;
  Arena arena;
  // pinned host staging for small D2H results (round messages, window sums)
  PinnedMem pinned{hipHostMallocCoherent | hipHostMallocMapped};
  int num_cus = 256;
  int wall_clock_khz = 100000;  // rate of wall_clock64() on the device
  double lasso_ms[LH_LASSO_NUM_PHASES] = {0};
  // one proof over several GPUs: host-side communicator + position of the shard bits
  lh_comm comm = {0, 1, nullptr, nullptr, nullptr};
  bool has_comm = false;
  bool comm_loopback = false;  // measurement aid: every peer is a copy of this rank (comm.cpp comm_attach_loopback)
  size_t shard_bit = 0;
  // a sharded proof is running on this ctx (set for the duration of lh_lasso_prove_sharded): every routine of the prover
  // then takes its tables as this rank's shards (struct Shard below); otherwise an attached communicator is ignored
  bool shard_active = false;
  void* rccl_comm = nullptr;      // ncclComm_t of the built-in RCCL backend (comm.cpp)
  DevMem comm_stage;              // device staging of host-side gathers over a device-only communicator
  uint64_t comm_stats[2] = {0, 0};  // collectives issued: device-side, host callback
  // the same by phase of the Lasso prove that issued them (index = the phase in progress: witness, commit, surge, leaves,
  // gkr, evals, open; 7 = outside a Lasso prove): [phase][0] collectives, [phase][1] bytes this rank contributed
  uint64_t comm_phase_stats[8][2] = {};
  int comm_phase = 7;
  // sharded sum-check rounds: the round kernel leaves its D sums in this DEVICE buffer (and "publishes" to a device
  // word) instead of pinned host memory; the all-gather and the sum-and-publish kernel follow on the stream
  Fr* sc_redirect = nullptr;
  uint64_t* sc_wide = nullptr;  // all-reduce variant: the round kernel also leaves its sums as tagged u64 lanes here (device)
  uint32_t sc_tag = 0;          // the tag of the round in progress (ScFinishArgs::tag)
  uint32_t sc_tag_seq = 0;      // tags handed out so far
  PinnedMem lanes_host{hipHostMallocCoherent | hipHostMallocMapped};  // where the all-reduce leaves the lanes' sums (created on first use)
  uint64_t* lanes_host_block();  // 128 words, zeroed when created
  bool comm_host_recv_ok = true;   // the attach-time probe (comm.cpp comm_probe_host_recv): RCCL delivers into pinned host memory here
  Fr* round_out(Fr* out_host) const { return sc_redirect ? sc_redirect : out_host; }
  void wait_round(uint32_t seq) {  // the host's wait for a round kernel's sums (nothing to wait for when they stay on the device)
    if (!sc_redirect) wait_flag(seq);
  }
  uint64_t* tail_trace = nullptr;  // development: device stamps of the last resident tail (LH_SC_TAIL_TRACE)
  // development (LH_HOST_TRACE=1): host wall-clock stamps at named points of a prove, printed (deltas in us) when the prove
  // ends - where the host's share of a gap between two kernels goes
  std::vector<std::pair<const char*, double>> host_stamps;
  bool host_trace_on = false;
  void host_stamp(const char* tag);
  void host_stamps_print();
  // eq tables of point tails y[1..n) built during one proof (sumcheck.cpp eq_half_*): an evaluation, a sum-check and the batch
  // opening at the same point share one table.  Arena memory of the proof's scope: the proof clears the list (EqHalfScope).
  struct EqHalfEntry {
    std::vector<uint8_t> key;  // the bytes of y[1..n)
    const Fr* table;
    bool sharded = false;  // this rank's shard of the table (sharded proofs)
  };
  std::vector<EqHalfEntry> eq_half_cache;
  // quad sums S_t = sum_q E_1[q] col[4q + t], t = 0..3, of 32-bit columns at points of one proof (sumcheck.cpp quad_sums_*): the
  // evaluation side makes them, the batch opening's column rounds take them.  Keyed by the column's device pointer, its length
  // and ALL coordinates of the point - the arena hands out the same pointers proof after proof -; same lifetime as the eq
  // tables above (EqHalfScope), cleared at the start of every prove.
  struct QuadSumEntry {
    const uint32_t* col;
    size_t len;
    std::vector<uint8_t> point;  // the bytes of y[0..n)
    Fr s[4];
  };
  std::vector<QuadSumEntry> quad_sums;
  bool prof = false;
  std::vector<ProfRec> prof_recs;
  // LIVE records (lh_profile_enable(ctx, 2)): a HIP-event pair around every bucket-accumulation launch, on the stream it is
  // launched on, nothing synchronised and nothing serialised - the timed region as it runs.  The two halves of a pipelined
  // MSM batch run at the same time on two streams, so a launch's duration is its SPAN (what a kernel trace shows too) and
  // the chip's rate follows from the batch's span (first start to last end): lh_profile_read resolves both.
  bool live = false;
  struct LiveRec {
    ProfRec rec;
    Event e0, e1;
    uint32_t batch;
  };
  std::vector<LiveRec> live_recs;
  std::vector<Event> live_pool;  // events not in use
  uint32_t live_batch = 0;
  Event live_event();
  void live_resolve(std::vector<ProfRec>& out);  // waits for the streams, appends per-launch and per-batch records, recycles the events
  // helper ctx (same device, own stream / arena / pinned blocks; dev.cpp ctx_helper) and what it is committing ahead of
  // the opening (open_columns.cpp open_precommit_*): both owned by this ctx
  bool is_helper = false;  // this ctx is somebody's helper: its throughput kernels leave wave slots to the owner's stream
  std::unique_ptr<Ctx> helper;
  OpenPrecommit* precommit = nullptr;
  std::unique_ptr<HostWorker> worker;  // the host thread that drives THIS ctx when it is somebody's helper (created on first use)
  Event handoff_ev{hipEventDisableTiming};  // recorded on this ctx's stream where a helper's stream may start reading its columns
  // a staged precommit (Options::open_precommit_stages): [0], [1] behind the commit batch's accumulation launches on the
  // stream and the aux stream - the helper's stage 1 waits for them -, [2] where the trees are built - its stage 2 does
  Event stage_ev[3] = {Event(hipEventDisableTiming), Event(hipEventDisableTiming), Event(hipEventDisableTiming)};
  // phase boundaries of the last Lasso prove as events on the stream (no host sync at a boundary: lasso.cpp lap)
  Event phase_ev[LH_LASSO_NUM_PHASES];
  bool phase_ev_pending = false;
  void phase_times_resolve();  // events -> lasso_ms (waits for the last one)
  Event prof_ev[2];
  // committed sparse polynomials (spark.cpp SparkPoly): device memory outside the arena, freed by lh_spark_free or with the ctx
  std::vector<struct SparkPoly*> spark_polys;
  // R1CS keys (spartan.cpp R1csKey): each owns three of the polynomials above and one device block of its own; freed by
  // lh_r1cs_free or with the ctx, before the polynomials
  std::vector<struct R1csKey*> r1cs_keys;
  void* pin(size_t bytes) { return pinned.reserve(bytes, 65536); }  // grows the pinned buffer if needed
  // small device -> host download through a second pinned staging buffer, synchronising: an async copy into
  // pageable memory makes the runtime pin pages on the fly (hundreds of microseconds for a few KB)
  PinnedMem stage{hipHostMallocCoherent | hipHostMallocMapped};
  // pinned staging of the radix sort's slab descriptors (sort.hip) and the event after their last upload
  PinnedMem sort_stage[2];
  Event sort_ev[2] = {Event(hipEventDisableTiming), Event(hipEventDisableTiming)};
  hipEvent_t sort_stage_done(int side) { return sort_ev[side].get(); }
  void d2h(void* dst, const void* d_src, size_t bytes);
  void sync() { LH_HIP(hipStreamSynchronize(stream)); }
  // Round-trip fast path: a kernel publishes its (small) result into pinned memory and then stores a
  // sequence number with system-scope release; the host spins on it instead of going through
  // hipStreamSynchronize (tens of microseconds per call, paid once per sum-check round).
  PinnedMem flag{hipHostMallocCoherent | hipHostMallocMapped};  // 64 words
  uint32_t flag_seq = 0;
  DevMem ticket;               // device counter for in-launch final reductions; only ever grows (word 8: device flag;
                               // word 10: the resident grand-product kernel's start verdict; words 32..47: the resident
                               // tail's relay chunks)
  uint32_t ticket_base = 0;    // its value before the next launch
  DevMem fin_lanes;  // ScFinishArgs::lanes: 8 lanes per partial sum, FIN_LANE_SUMS of them; zeroed once, then only tagged lanes
  // a second stream of the ctx for work that runs BESIDE the ctx's stream inside one call (msm.hip: the tails of a batch's
  // first half); its kernels draw tickets from word 16 and publish to flag word 4, so the two streams never share a counter
  Stream aux_stream;
  Event aux_ev{hipEventDisableTiming};
  uint32_t aux_ticket_base = 0;
  void aux_streams();  // creates them on first use
  struct ScFinishArgs finish_for_aux(uint32_t grid, uint32_t seq);
  void wait_flag_aux(uint32_t seq);
  // (`stored_bytes`: what the launch's workgroups store besides their sums - LH_FIN_LANES_MIN_BYTES, development)
  struct ScFinishArgs finish_for(uint32_t grid, Fr* out_host, uint32_t seq, double stored_bytes = 0);
  uint32_t next_seq() { return ++flag_seq; }
  // host -> resident kernel mailbox (second cache line of the flag allocation)
  struct TailMbox* mbox() { return (struct TailMbox*)(flag.as<char>() + 64); }
  void mbox_send(const Fr& r, uint32_t seq);
  void mbox_abort();
  // the resident grand-product kernel's boxes (kernels_gkr.hip): host -> kernel layer messages (pinned) and the device
  // relay of whatever one workgroup fetched from the host; created on first use
  PinnedMem gkr_mbox{hipHostMallocCoherent | hipHostMallocMapped};
  DevMem gkr_relay;
  void gkr_boxes();
  void gkr_send_layer(const Fr* vals, size_t count, uint32_t seq);
  void gkr_abort();   // mbox_abort + the layer box
  void gkr_resync();  // after an aborted launch: markers cleared, ticket counter re-read
  void wait_flag(uint32_t seq);
  // more than 64 KB of dynamic LDS for `fn` on this ctx's device (the attribute is per device: once per ctx and kernel)
  std::vector<const void*> lds_opted;
  void opt_in_lds(const void* fn, int bytes);
  // message of a resident tail round: `count` chunks that all carry `seq` -> `count` / 3 field elements
  void wait_chunks(const struct TailChunk* chunks, size_t count, uint32_t seq, Fr* out);
  // the same; false (nothing copied) when the first chunk carries `alt` instead
  bool wait_chunks_or(const struct TailChunk* chunks, size_t count, uint32_t seq, uint32_t alt, Fr* out);
};

// The host's half of a round kernel's hand-off (round.cuh), for the duration of one k_* wrapper: takes the round's
// sequence number, opens an arena scope, redirects the output of a sharded round (Ctx::sc_redirect); hand_off() then
// chooses `partials` - the output buffer itself when the launch is one workgroup with one slot of sums, arena memory
// otherwise - and makes the kernel's ScFinishArgs; wait() is the host's wait for the sums.
struct RoundLaunch {
  Ctx& c;
  const uint32_t seq;
  ArenaScope scope;
  Fr* const out;  // where the launch's sums go
  Fr* partials = nullptr;
  ScFinishArgs fin;
  RoundLaunch(Ctx& c_, Fr* out_host) : c(c_), seq(c_.next_seq()), scope(c_.arena), out(c_.round_out(out_host)) {}
  // `grid` workgroups that leave `slots` x `sums` partial sums each (slots > 1: finish_round_waves, whose single workgroup
  // still draws a ticket - which finish_for does not count)
  void hand_off(size_t grid, size_t sums, double stored_bytes = 0, size_t slots = 1) {
    partials = grid * slots == 1 ? out : c.arena.alloc_n<Fr>(grid * slots * sums);
    fin = c.finish_for((uint32_t)grid, out, seq, stored_bytes);
    if (grid == 1 && slots > 1) c.ticket_base += 1;
  }
  void wait() { c.wait_round(seq); }
};

struct ShardActive {  // Ctx::shard_active for the duration of one sharded prove, whatever way it ends
  Ctx& c;
  explicit ShardActive(Ctx& c_) : c(c_) { c.shard_active = true; }
  ~ShardActive() { c.shard_active = false; }
};

// Geometry of a proof sharded over R = 2^rho ranks.  A table of 2^m entries is split on the index bits
// [j, j + rho): rank s holds the 2^(m - rho) entries (hi || lo) <-> global index (hi, s, lo).  Every kernel is
// index-agnostic over such a local table because
//   * sum-check pairs are (2b, 2b+1): bit 0, local while it is not a shard bit (rounds 0..j-1);
//   * product-tree / quotient halves are split on the top bit, local while the table has more than j + rho variables.
// `on` false (no sharded proof running): rho = 0 and nothing is sharded - the single-GPU prover is the world of one.
struct Shard {
  bool on = false;
  bool loopback = false;  // the measurement communicator (every peer is a copy of this rank)
  size_t rho = 0, j = 0, rank = 0, R = 1;
  explicit Shard(const Ctx& c) {
    if (!c.shard_active) return;
    on = true, j = c.shard_bit, rank = (size_t)c.comm.rank, R = (size_t)c.comm.size, loopback = c.comm_loopback;
    while (((size_t)1 << rho) < R) rho++;
  }
  // is a table of `num_vars` variables held in shards?  Smaller ones are replicated and worked on redundantly.  (A
  // communicator of ONE rank goes through the same code paths - its "exchange" round still needs one round before it.)
  bool sharded(size_t num_vars) const { return on && num_vars >= j + (rho ? rho : 1) + 1; }
  size_t local_vars(size_t num_vars) const { return sharded(num_vars) ? num_vars - rho : num_vars; }
  size_t local_len(size_t num_vars) const { return (size_t)1 << local_vars(num_vars); }
};

// A REPLICATED array of `len` entries (final_cts, a quotient level below the replication point) whose MSM every rank would
// repeat: an MSM is additive over point ranges (the chunk-then-sum of util/arithmetic/msm.rs:101-114), so rank s takes the
// entries [first, first + count) = [s len / R, (s + 1) len / R) and the partial commitments are added over the ranks.
// Arrays shorter than the world go to rank 0 whole; outside a sharded proof the range is the whole array.
struct ReplicatedRange {
  size_t first = 0, count = 0;
  ReplicatedRange(const Shard& sh, size_t len) {
    if (!sh.on || sh.R <= 1) {
      count = len;
    } else if (len < sh.R) {
      // (over the loopback communicator "the sum over the ranks" is R copies of this rank's part: a part that is empty on
      // every rank but 0 would make the sum the identity there, which no transcript can carry - a handful of points)
      count = sh.rank == 0 || sh.loopback ? len : 0;
    } else {
      const size_t per = len / sh.R;  // (len and R are powers of two in every use; a remainder would go to the last rank)
      first = sh.rank * per;
      count = sh.rank + 1 == sh.R ? len - first : per;
    }
  }
};

// Persistent host worker threads for the short host-side tails (window combines of an MSM batch): spawning
// std::threads per call costs ~50 us each, more than the work itself.
void host_parallel_for(size_t n, const std::function<void(size_t)>& fn);
// a host_parallel_for over about n items follows within `us` microseconds: wake that many workers now and let them poll
// for it (the poster otherwise pays the sleepers' wake-up, ~50 us, on the critical path between two kernels)
void host_parallel_prewake(size_t n, unsigned us);

struct ProfScope {
  Ctx& c;
  ProfRec rec;
  bool on;
  ProfScope(Ctx& c_, const char* name, double bytes, double muls, double items) : c(c_), on(c_.prof) {
    if (!on) return;
    snprintf(rec.name, sizeof rec.name, "%s", name);
    rec.bytes = bytes, rec.muls = muls, rec.items = items, rec.ms = 0;
    (void)c.prof_ev[1].get();  // (both exist from here on: the destructor creates nothing)
    LH_HIP(hipEventRecord(c.prof_ev[0].get(), c.stream));
  }
  ~ProfScope() {
    if (!on) return;
    (void)hipEventRecord(c.prof_ev[1].get(), c.stream);
    (void)hipEventSynchronize(c.prof_ev[1].get());
    float ms = 0;
    (void)hipEventElapsedTime(&ms, c.prof_ev[0].get(), c.prof_ev[1].get());
    rec.ms = ms;
    c.prof_recs.push_back(rec);
  }
};

// ------------------------------------------------------------------ kernel launchers (kernels_poly.hip)
void k_fr_from_u64(Ctx&, const uint64_t* in, size_t n, Fr* out);
void k_fr_from_u32(Ctx&, const uint32_t* in, size_t n, Fr* out);
void k_fr_to_repr(Ctx&, const Fr* in, size_t n, Fr* out);
void k_fr_from_repr(Ctx&, const Fr* in, size_t n, Fr* out);
void k_fr_binop(Ctx&, int op, const Fr* a, const Fr* b, size_t n, Fr* out);  // 0 add 1 sub 2 mul
void k_fr_mul_chain(Ctx&, const Fr* a, const Fr* b, size_t n, int iters, Fr* out);
void k_fr_batch_invert(Ctx&, const Fr* in, size_t n, Fr* out);
void k_fix_var(Ctx&, const Fr* in, size_t n_in, const Fr& x, Fr* out);
// binds `count` tables of n_in entries each in one launch
void k_fix_var_multi(Ctx&, const Fr* const* in, Fr* const* out, size_t count, size_t n_in, const Fr& x);
void k_eq_xy(Ctx&, const Fr* y, size_t num_vars, Fr* out);  // y: host array
// out_host (pinned) [i] = in[i][0] + (in[i][1] - in[i][0]) * x ; synchronises
void k_bind_first(Ctx&, const Fr* const* in, size_t count, const Fr& x, Fr* out_host);
// out_host (pinned) [i*k + j] = in[i][j], j < k ; synchronises
void k_gather_heads(Ctx&, const Fr* const* in, size_t count, int k, Fr* out_host);
void k_lincomb(Ctx&, const Fr* const* polys, const Fr* w, size_t count, size_t n, Fr* out);
// out[b] = lo + x (hi - lo), lo = sum_k w_k p_k[b], hi = sum_k w_k p_k[b + half]
void k_lincomb_fold(Ctx&, const Fr* const* polys, const Fr* w, size_t count, size_t half, const Fr& x, Fr* out);
// the same first step of g = sum_k coef_k col_k over 32-bit columns (entries beyond lens[k] are zero); false: too many columns
bool k_lincomb_fold_small(Ctx&, const uint32_t* const* cols, const size_t* lens, const Fr* coef, size_t count, size_t half,
                          const Fr& x, Fr* out);
// out[i] = <polys[i], weights>, i < count ; result on host
void k_inner_products(Ctx&, const Fr* const* polys, size_t count, const Fr* weights, size_t n, Fr* out_host);
// the most inputs a launch of the 32-bit column kernels takes (their argument blocks travel through memory)
constexpr int LCM_MAX_FR = 8, LCM_MAX_SMALL = 24;  // k_lincomb_mixed
constexpr int LCF_MAX = 24;                        // k_lincomb_fold_small
constexpr int LCB_MAX = 24;                        // k_lincomb_bind2
// small-valued columns without their field-element views: 8 multiply-adds per term into a wide accumulator
void k_inner_products_small(Ctx&, const uint32_t* const* polys, size_t count, const Fr* weights, size_t n, Fr* out_host);
// the same against eq(y) given as the eq table of y[1..] (`half` entries) and y0
void k_inner_products_small_half(Ctx&, const uint32_t* const* polys, size_t count, const Fr* eq_half, size_t half,
                                 const Fr& y0, Fr* out_host);
// An eq-factored degree-2 sum-check over ONE table that still is a 32-bit column (Surge over the output column, lasso.cpp):
// out_host[0..3] = sum_b e0[b] col[2b], sum_b e0[b] col[2b+1], sum_q (e0[2q] + e0[2q+1]) col[4q+2], the same with col[4q+3]
// (the claim's two halves - and the sums of rounds 0 and 1), b < 2 quads, q < quads
void k_inner_products_small_quads(Ctx&, const uint32_t* col, const Fr* e0, size_t quads, Fr* out_host);
// d_out[4 k + t] (DEVICE, queued on the stream) = sum_q e1[q] cols[k][4 q + t], t = 0..3, q < quads; lens: multiples of 4
void k_inner_products_quads(Ctx&, const uint32_t* const* cols, const size_t* lens, size_t count, const Fr* e1, size_t quads,
                            Fr* d_out);
// the same sums of ALL the columns in one launch (per QS_MAX_COLS) against one read of e0 = the eq table of the point's tail
// y[1..] (2 quads entries): d_out[4 k + t] (DEVICE, queued on the stream) = sum_q (e0[2q] + e0[2q+1]) cols[k][4 q + t]
constexpr int QS_MAX_COLS = 24;
void k_quad_sums(Ctx&, const uint32_t* const* cols, const size_t* lens, size_t count, const Fr* e0, size_t quads, Fr* d_out);
// out[i] = sum_k w[k] (cols[k][4i..4i+3] bound with (r0, r1)), i < 2 size; out_host[e] = sum_b eq_level[b] out[2b + e]
void k_lincomb_bind2(Ctx&, const uint32_t* const* cols, const size_t* lens, const Fr* w, size_t count, const Fr& r0, const Fr& r1,
                     const Fr* eq_level, size_t size, Fr* out, Fr* out_host);
// round 2 binds r0 and r1 at once: out[i] = the column's entries 4i..4i+3 bound with (r0, r1), i < 2 size;
// out_host[0] = sum_b eq_level[b] out[2b+1]
void k_sc_round_u32_bind2(Ctx&, const uint32_t* col, const Fr* eq_level, const Fr& r0, const Fr& r1, size_t size, Fr* out,
                          Fr* out_host);
// out[i] = sum_k wfr[k] fr[k][i] + sum_k wsm[k] sm[k][i], i < n; u32 column k has sm_len[k] entries (zero beyond)
void k_lincomb_mixed(Ctx&, const Fr* const* fr, const Fr* wfr, size_t num_fr, const uint32_t* const* sm,
                     const size_t* sm_len, const Fr* wsm, size_t num_sm, size_t n, Fr* out);
// product tree level: out[i] = in[i] * in[half + i]
void k_tree_up(Ctx&, const Fr* in, size_t half, Fr* out);
void k_tree_up_multi(Ctx&, const Fr* const* in, Fr* const* out, size_t count, size_t half);
// every level above level H[i] (2^(H+1) nodes at in[i], H <= 9) of `count` product trees, one launch:
// level h < H lands at out[i] + (2^(h+1) - 2)
void k_tree_tops(Ctx&, const Fr* const* in, Fr* const* out, const int* H, size_t count);
// fractional layer: (p_l q_r + p_r q_l, q_l q_r)
void k_frac_up(Ctx&, const Fr* p, const Fr* q, size_t half, Fr* vp, Fr* vq);
// KZG quotient step at level i: q = hi - lo ; lo' = lo + (hi - lo) * x
void k_quotient_step(Ctx&, const Fr* rem, size_t half, const Fr& x, Fr* q, Fr* rem_out);
// Lasso fingerprints: rs = dim*g2 + e*g + ts - tau ; ws = rs + 1
void k_lasso_rw_leaves(Ctx&, const uint32_t* dim, const uint32_t* e, const uint32_t* ts, size_t n,
                       const Fr& gamma, const Fr& gamma2, const Fr& tau, Fr* rs, Fr* ws);
// the same plus the level above the leaves of both trees (rs_up[i] = rs[i] * rs[i + n/2], n/2 entries each)
void k_lasso_rw_leaves_up(Ctx&, const uint32_t* dim, const uint32_t* e, const uint32_t* ts, size_t n, const Fr& gamma,
                          const Fr& gamma2, const Fr& tau, Fr* rs, Fr* ws, Fr* rs_up, Fr* ws_up);
// the read / write leaves of ALL memories of a batch proof (lasso.cpp lasso_prove_batch) in one launch, the memory index in
// blockIdx.y: per memory the three u32 columns and where its leaves go.  `up`: the level above the leaves comes with them
// as in k_lasso_rw_leaves_up (rs_up / ws_up: n / 2 nodes each; ws[m] may then be null: the write leaves are not stored);
// otherwise rs_up / ws_up are not read.  All memories have n entries.
constexpr int LASSO_RW_BATCH_MAX = 8;
struct LassoRwBatch {
  const uint32_t *dim[LASSO_RW_BATCH_MAX], *e[LASSO_RW_BATCH_MAX], *ts[LASSO_RW_BATCH_MAX];
  Fr *rs[LASSO_RW_BATCH_MAX], *ws[LASSO_RW_BATCH_MAX], *rs_up[LASSO_RW_BATCH_MAX], *ws_up[LASSO_RW_BATCH_MAX];
};
void k_lasso_rw_leaves_batch(Ctx&, const LassoRwBatch& p, size_t num_memories, size_t n, bool up, const Fr& gamma,
                             const Fr& gamma2, const Fr& tau);
// init = m*g2 + T[m]*g - tau ; fin = init + final_cts[m]
void k_lasso_if_leaves(Ctx&, int subtable, uint32_t chunk_bits, const uint32_t* final_cts, size_t m,
                       const Fr& gamma, const Fr& gamma2, const Fr& tau, Fr* init, Fr* fin, const uint32_t* tab = nullptr);
// Lasso witness: counters and subtable reads
// keep_sorted / keep_index (optional, n entries each): the column sorted by value and the positions it came from
// OR of all entries of every column (its bit length bounds the values); synchronises
void k_or_u32(Ctx&, const uint32_t* const* cols, size_t count, size_t n, uint32_t* out_host);
void k_fill_u32(Ctx&, uint32_t* out, uint32_t value, size_t n);
// out[i] = a[i] | b[i] << shift
void k_pack_u32(Ctx&, const uint32_t* a, const uint32_t* b, uint32_t shift, size_t n, uint32_t* out);
// v = col[i + half] - col[i] + offset (entries beyond `len` are zero; 0 < v < 2^33): out_lo[i] = v, or with out_hi:
// out_lo[i] = v & 0xffff, out_hi[i] = v >> 16
void k_delta_u32(Ctx&, const uint32_t* col, size_t len, size_t half, uint64_t offset, uint32_t* out_lo, uint32_t* out_hi);
// access counters of all `cc` chunk columns (n lookups into m cells each) in one launch set, one bad-index readback per call;
// keep_sorted / keep_index: null, or per column where to leave the sorted values and their positions
void k_lasso_counters(Ctx&, const uint32_t* const* dims, size_t cc, size_t n, size_t m, uint32_t* const* read_ts,
                      uint32_t* const* final_cts, uint32_t* const* keep_sorted = nullptr, uint32_t* const* keep_index = nullptr);
// the sharded counters' steps (lasso.cpp lasso_counters_sharded), ALL `cc` chunk columns per call: partition the local
// lookups by address owner (sidx[q]: local indices in send order; send[q]: (address on the owner) << hi_bits | local index >>
// shard_bit; start_host[q * (R + 1) + o]: first send position of owner o in column q), rank the received lookups on the
// owner (recv[q]: n_recv[q] keys, one segment per sender; counts: cc * m_loc), scatter the returned ranks, assemble final_cts
void k_cs_partition(Ctx&, const uint32_t* const* dims, size_t cc, size_t n, size_t m, unsigned rho, unsigned j, unsigned hi_bits,
                    uint32_t* const* sidx, uint32_t* const* send, uint32_t* start_host, bool* bad_out);
void k_cs_rank(Ctx&, const uint32_t* const* recv, const size_t* n_recv, size_t cc, unsigned hi_bits, unsigned a_bits, size_t m_loc,
               uint32_t* const* ret, uint32_t* counts);
void k_cs_scatter(Ctx&, const uint32_t* const* back, const uint32_t* const* sidx, size_t cc, size_t n, uint32_t* const* read_ts);
void k_cs_final(Ctx&, const uint32_t* all_counts, size_t cc, size_t m, unsigned rho, size_t m_loc, uint32_t* const* final_cts);
// (tab: the device entries of a registered subtable - a masked gather; null: the built-in kind's computed entry)
void k_lasso_subtable_read(Ctx&, int subtable, uint32_t chunk_bits, const uint32_t* dim, size_t n, uint32_t* e,
                           const uint32_t* tab = nullptr);
// a[k] = g(E_0[k],..): small-integer evaluation into Fr
struct LassoG {
  uint32_t num_terms;
  Fr coeff[LH_LASSO_MAX_TERMS];
  uint8_t nfac[LH_LASSO_MAX_TERMS];
  uint8_t fac[LH_LASSO_MAX_TERMS][LH_SC_MAX_FACTORS];
  const uint32_t* e[LH_LASSO_MAX_MEMORIES];
};
void k_lasso_output(Ctx&, const LassoG& g, size_t n, Fr* a);
struct LassoGSmall {  // g = sum_t coeff[t] * E_{fac[t]} with 32-bit coefficients and a value that fits 32 bits
  uint32_t num_terms;
  uint32_t coeff[LH_LASSO_MAX_TERMS];
  uint8_t fac[LH_LASSO_MAX_TERMS];
  const uint32_t* e[LH_LASSO_MAX_MEMORIES];
};
void k_lasso_output_small(Ctx&, const LassoGSmall& g, size_t n, uint32_t* a);
// g with product terms whose largest value fits 32 bits (lasso.cpp: the bound from the subtables' widths - the comparison
// and equality tables): integer products of the 32-bit reads, no partial product can exceed the bound
struct LassoGSmallProd {
  uint32_t num_terms;
  uint32_t coeff[LH_LASSO_MAX_TERMS];
  uint8_t nfac[LH_LASSO_MAX_TERMS];
  uint8_t fac[LH_LASSO_MAX_TERMS][LH_SC_MAX_FACTORS];
  const uint32_t* e[LH_LASSO_MAX_MEMORIES];
};
void k_lasso_output_small_prod(Ctx&, const LassoGSmallProd& g, size_t n, uint32_t* a);
// canonical value of every entry as u32; false if an entry is not below 2^bits
bool k_fr_to_index(Ctx&, const Fr* in, size_t n, uint32_t bits, uint32_t* out);
// both tables hold Montgomery residues in [0, r): equal values have equal limbs
bool k_fr_tables_equal(Ctx&, const Fr* a, const Fr* b, size_t n);

// ------------------------------------------------------------------ communicator (comm.cpp)
void rccl_unique_id(uint8_t out[LH_RCCL_UNIQUE_ID_BYTES]);
void comm_attach_rccl(Ctx&, int rank, int size, const uint8_t id[LH_RCCL_UNIQUE_ID_BYTES], size_t shard_bit);
void comm_probe_host_recv(Ctx&);  // attach-time self-test of the all-reduce into pinned host memory (sets Ctx::comm_host_recv_ok)
void comm_attach_loopback(Ctx&, int rank, int size, size_t shard_bit);
void comm_detach(Ctx&);
// recv = size * bytes, rank-major.  _dev: device buffers, enqueued on the ctx's stream (staged through the host when
// the communicator has no device collective); _host: host buffers, synchronous
void comm_all_gather_dev(Ctx&, const void* d_send, void* d_recv, size_t bytes);
void comm_all_gather_host(Ctx&, const void* send, void* recv, size_t bytes);
// personalised exchange of `nbuf` device buffers at once (elements of `elem` bytes; the chunk columns of the sharded access
// counters): from buffer b this rank sends send_cnt[b * R + p] elements at d_send[b] + send_off[b * R + p] to every peer p and
// receives recv_cnt[b * R + p] from it at d_recv[b] + recv_off[b * R + p] - ONE collective (RCCL: one group of sends and
// receives).  peer_off[b * R + p]: where, inside p's send buffer b, the segment for this rank starts; the send buffers are
// slices of ONE allocation, buffer b at send_base + b * send_stride elements, the same stride on every rank - both only used
// by transports without point-to-point sends (the whole allocation is staged through an all-gather).
void comm_all_to_all_multi(Ctx&, size_t nbuf, const void* const* d_send, const size_t* send_off, const size_t* send_cnt,
                           void* const* d_recv, const size_t* recv_off, const size_t* recv_cnt, const size_t* peer_off,
                           const void* send_base, size_t send_stride, size_t elem);
// v[i] = sum over the ranks of v[i], `count` field elements in a device buffer the ctx's stream owns; the sums are left in
// out_host (pinned) followed by the flag `seq` (the closing steps of a sharded sum-check round)
void comm_sum_publish(Ctx&, const Fr* d_part, Fr* d_scratch, size_t count, Fr* out_host, uint32_t seq);
// the all-reduce variant of the same step (Options::comm_round 1 / 2): d_lanes = the 8 * count tagged u64 lanes the round
// kernel left (ScFinishArgs::wide, tag = c.sc_tag); ONE collective adds them over the ranks into pinned host memory, the
// host waits until every lane carries the ranks' tags and reduces mod r.  Synchronous: out_host holds the sums on return.
void comm_sum_lanes(Ctx&, uint64_t* d_lanes, uint64_t* d_scratch, size_t count, Fr* out_host);
// a fresh tag for the next all-reduce round (never 0, below 2^24 / R)
uint32_t comm_next_tag(Ctx&);
// loopback all-reduce: out[i] = in[i] * R (every peer is a copy of this rank), one launch (kernels_poly.hip)
void k_loopback_allreduce_lanes(Ctx&, const uint64_t* d_in, size_t n, size_t R, uint64_t* out);

// ------------------------------------------------------------------ sharding helpers (kernels_poly.hip)
// inverse of k_shard_extract over the all-gathered shards: global[g] = gathered[s(g) * n_local + local(g)]
void k_shard_merge(Ctx&, const void* gathered, size_t n_local, size_t j, size_t rho, size_t elem, void* global);
// out[t][(hi * R + s) * block + lo] = gathered[(s * count + t) * n_local + hi * block + lo]: the residual tables of a
// sharded sum-check (block = 1 once the shard bits have reached bit 0) or tree levels / remainders at the replication
// point (block = n_local: concatenation)
void k_gather_interleave(Ctx&, const Fr* gathered, size_t count, size_t n_local, size_t R, size_t block, Fr* const* out);
// out_host[x] = sum_s all[s * D + x], x < D; then the flag: the closing step of a sharded sum-check round
void k_sum_publish(Ctx&, const Fr* all, size_t R, size_t D, Fr* out_host, uint32_t seq);
// local[idx] = global[((idx >> j) << (j + rho)) | (s << j) | (idx & (2^j - 1))], elements of `elem` bytes (4, 32, 64)
void k_shard_extract(Ctx&, const void* global, size_t n_local, size_t j, size_t rho, size_t s, size_t elem, void* local);
// the loopback communicator's all-gather: recv block s = send rotated by 32 s bytes (comm.cpp), one launch
void k_loopback_gather(Ctx&, const void* d_send, void* d_recv, size_t bytes, size_t R);
// out[i] = in[i] * w
void k_scale(Ctx&, const Fr* in, const Fr& w, size_t n, Fr* out);

// ------------------------------------------------------------------ sum-check round (kernels_sumcheck.hip)
constexpr int SC_MAX_TABLES = 72;  // 32 product trees (8 memories) + eq fit one GKR batch; kernel arguments stay < 4 KB
struct ScRound {
  // tables of the current round: BIND ? 4*size entries in, 2*size out : 2*size entries in
  const Fr* in[SC_MAX_TABLES];
  Fr* out[SC_MAX_TABLES];
  uint32_t num_tables;
  uint32_t num_terms;
  int32_t global_eq;  // table id multiplied onto the sum, or -1
  Fr coeff[LH_SC_MAX_TERMS];
  uint8_t coeff_is_one[LH_SC_MAX_TERMS];
  uint8_t nfac[LH_SC_MAX_TERMS];
  uint8_t fac[LH_SC_MAX_TERMS][LH_SC_MAX_FACTORS];
  Fr r;  // challenge of the previous round (BIND only)
  // "eq factoring" (sumcheck.cpp): when set, global_eq is -1 and the eq factor of the expression is eq_level[b], the eq
  // table over the variables AFTER this round's; the kernel returns q(X) = sum_b eq_level[b] * g(X, b)
  const Fr* eq_level;
  // product-pair shape (every term coeff_m * l_m * r_m over 2 num_terms distinct tables, factored eq; the generic layers of
  // the grand products): 1 = the factored degree-2 rounds run sc_round_pp_kernel (four products per Montgomery reduction);
  // 2 = this BIND round also FOLDS the coefficients into the left factors (l'_m = coeff_m l_m is what it stores: the
  // caller treats the coefficients as one from then on and divides them out of the final evaluations)
  uint8_t pp;
};
// evals_host[0..degree) receives sum_b expr at X = 1..degree (X = 0 is derived by the caller)
// -> the launch it chose folded the coefficients into the left factors (ScRound::pp == 2 and a kernel that does fold)
bool k_sc_round(Ctx&, const ScRound& rd, int degree, bool bind, size_t size, Fr* evals_host);
// true when k_sc_round would run the streaming one-thread-per-pair kernel for this shape (not the LDS-staged one)
bool k_sc_round_streams(const ScRound& rd, int degree, size_t size);
// out[i] = in[2 i] + in[2 i + 1]: the eq table over one variable less (eq factoring)
// levels[k] = pair sums of levels[k - 1] (levels[-1] = `in`, n_in entries, a power of two), k < nlev: the levels of a
// factored eq table (host.hpp EqFactoring), 9 per launch
void k_eq_levels(Ctx&, const Fr* in, size_t n_in, Fr* const* levels, size_t nlev);
// Batch-opening shape sum_m eq_m * poly_m with every eq factored: per term q_m(0) = sum_b E_m[b] v0, q_m(1) = sum_b E_m[b] v1
constexpr int SC_OPEN_MAX_TERMS = 6;
struct ScOpenRound {
  const Fr* in[SC_OPEN_MAX_TERMS];
  Fr* out[SC_OPEN_MAX_TERMS];
  const Fr* eq_level[SC_OPEN_MAX_TERMS];
  uint32_t num_terms;
  Fr r;
};
// out_host[2 m], out_host[2 m + 1] = q_m(0), q_m(1)
void k_sc_round_open(Ctx&, const ScOpenRound& rd, bool bind, size_t size, Fr* out_host);

// Streaming round of a grand-product layer whose trees come in pairs (A_i, A_i + 1) - Lasso's read set and write set at
// the leaf level, write = read + 1 entry by entry, and binding keeps the "+ 1".  With cs_i = c_A + c_B, k_i = c_B / cs_i:
//   c_A l r + c_B (l + 1)(r + 1) = cs_i (l + k_i)(r + k_i) + const_i
// so only the A tables are read and bound and a pair of trees costs one product per point.  Factored eq (eq_level as in
// ScRound); out_host[x - 1] = sum_b eq_level[b] * sum_i cs_i (l_i + k_i)(r_i + k_i) at X = x, x = 1, 2 (the caller adds
// the constants).
constexpr int SC_RW_MAX_PAIRS = 8;
struct ScRwRound {
  const Fr* l[SC_RW_MAX_PAIRS];
  const Fr* r[SC_RW_MAX_PAIRS];
  Fr* lo[SC_RW_MAX_PAIRS];
  Fr* ro[SC_RW_MAX_PAIRS];
  Fr cs[SC_RW_MAX_PAIRS], k[SC_RW_MAX_PAIRS];
  const Fr* eq_level;
  Fr rchal;
  uint32_t num_pairs;
};
// fold (BIND rounds): store l' = cs (l + k), r' = r + k instead of the bound l, r - the later rounds are ScRound::pp ones
void k_sc_round_rw(Ctx&, const ScRwRound& rd, bool bind, size_t size, Fr* out_host, bool fold = false);

// Resident tail: once the live tables of a sum-check fit the LDS of a few CUs, ONE launch runs all remaining rounds.
// G workgroups each keep a contiguous slice of every table in LDS (binding never crosses a slice); per round every
// workgroup leaves its D partial sums in device memory and draws a ticket, the one that draws the last ticket adds
// them up and sends the message to the host; when a slice is down to one entry the slices are handed (through device
// memory, same ticket protocol) to the workgroup that arrives last, which runs the remaining log2(G) rounds alone.
// Host <-> kernel traffic is self-validating 16-byte chunks {seq, 3 limbs} (TailChunk): a chunk is written with ONE
// 16-byte store and read with ONE 16-byte load on either side, so a message needs no flag and no fence (one PCIe
// crossing per direction and round instead of two).  After the last challenge the kernel publishes the final
// evaluation of the first `num_out` tables (plain values, flag = seq0 + rounds).
// No launch and no completion latency per round, tables never leave LDS.
struct TailChunk {
  uint32_t w[4];  // {seq, limb 3j, limb 3j+1, limb 3j+2} (chunk j = 0..2 of a field element; the last holds two limbs)
};
struct TailMbox {      // pinned, written by the host only: the challenge of round i carries seq0 + i in every chunk;
  TailChunk c[3];      // SC_TAIL_ABORT makes the kernel exit
  uint32_t pad[4];
};
constexpr uint32_t SC_TAIL_ABORT = 0xffffffffu;
constexpr int SC_TAIL_MAX_DEGREE = 6;
// largest resident table length (power of two, 0 = tail not applicable) for this expression
size_t k_sc_tail_capacity(const Ctx&, const ScRound& rd, int degree);
// rd.in: entry tables; first_bind: they hold 2*n0 entries and are bound with rd.r first.  Returns immediately.
// msg_host: 3 * degree chunks (value x at chunks 3x..3x+2), out_host: num_out field elements.
void k_sc_tail_launch(Ctx&, const ScRound& rd, int degree, size_t n0, bool first_bind, size_t num_out, uint32_t seq0,
                      TailChunk* msg_host, Fr* out_host);
// after a tail that ended early: the ticket counter is wherever the workgroups left it
void k_sc_tail_resync(Ctx&);

// ------------------------------------------------------------------ resident grand-product layers (kernels_gkr.hip)
// The layers of a product-tree argument (prove_grand_product) whose tables fit on-chip, in ONE launch: layer loop, eq
// tables and rounds inside the kernel, host <-> kernel traffic in TailChunk messages.  Per layer the host sends
// [c_0 .. c_{B-1}, y_0 .. y_{h-1}] (sequence number `seq`), the kernel answers every round j with q(1), q(2) of the
// eq-factored round polynomial (seq + 1 + j; the challenge comes back under the same number through the ctx's TailMbox)
// and ends the layer with the 2 B final evaluations (l'_k = c_k l_k and r_k per tree; flag = seq + h + 1).
constexpr int GKR_MAX_TREES = 16;
constexpr int GKR_MAX_VARS = 16;          // a resident layer has at most GKR_MAX_VARS - 2 variables
constexpr uint32_t GKR_CAP = 128;         // entries of a table one workgroup holds
constexpr uint32_t GKR_THREADS = 256;
constexpr uint32_t GKR_MSG_CHUNKS = 3 * (GKR_MAX_TREES + GKR_MAX_VARS);
constexpr uint32_t GKR_START_FAILED = 0xfffffffeu;  // first message chunk: the workgroups did not all start (see the kernel)
// A layer can also be the TAIL of a sum-check that ran its first rounds elsewhere (GKR_F_* flags): the tables come as
// separate left / right pointers, possibly still to be bound with the previous challenge, the eq level of the first
// resident round is read from memory, the coefficients (and the constant offsets of the read/write leaf layer,
// cs (l + k)(r + k)) come with the descriptor instead of a layer message.
enum { GKR_F_SPLIT = 1, GKR_F_BIND = 2, GKR_F_EQ = 4, GKR_F_NOMSG = 8, GKR_F_KOFF = 16 };
struct GkrLayerDev {
  const Fr* lv[GKR_MAX_TREES];  // the level of tree k: 2^(h + 1) nodes, left factors first (GKR_F_SPLIT: the left table)
  const Fr* rv[GKR_MAX_TREES];  // GKR_F_SPLIT: the right table
  uint32_t h, B;                // variables of the layer's tables, trees
  uint32_t g, s_log;            // g workgroups x 2^s_log entries = 2^h
  uint32_t seq;
  uint32_t flags;
  const Fr* eq_level;           // GKR_F_EQ: E of the first round, 2^(h - 1) entries
  Fr r_prev;                    // GKR_F_BIND: the tables hold 2^(h + 1) entries and are bound with this first
  Fr coef[GKR_MAX_TREES];       // GKR_F_NOMSG: the coefficients c_k
  Fr koff[GKR_MAX_TREES];       // GKR_F_KOFF: l'_k = c_k (l_k + koff_k), r'_k = r_k + koff_k
};
bool k_gkr_resident_geometry(uint32_t h, uint32_t* g, uint32_t* s_log);
// returns immediately; msg_host: 6 chunks, out_host: 2 * GKR_MAX_TREES field elements (pinned)
void k_gkr_resident_launch(Ctx&, const GkrLayerDev* layers, size_t num_layers, TailChunk* msg_host, Fr* out_host);

// ------------------------------------------------------------------ general expressions (kernels_expr.hip)
struct ExtRound {
  const Fr* in[SC_MAX_TABLES];
  Fr* out[SC_MAX_TABLES];
  uint32_t num_tables, num_terms;
  // device arrays, constant over the rounds of one sum-check
  const Fr* coeff;          // [num_terms]
  const uint8_t* is_one;    // [num_terms]
  const uint32_t* off;      // [num_terms + 1] into fac / store
  const uint8_t* fac;       // table ids
  const uint8_t* store;     // first occurrence of a table stores its bound pair
  Fr r;
};
void k_sc_round_ext(Ctx&, const ExtRound& rd, int degree, bool bind, size_t size, Fr* evals_host);
void k_rotate_gather(Ctx&, const Fr* poly, size_t num_vars, int rot, uint32_t primitive, uint32_t x_inv, Fr* out);
void k_identity_table(Ctx&, size_t n, Fr* out);
void k_identity_table_shard(Ctx&, size_t n_local, size_t j, size_t rho, size_t rank, Fr* out);
// BooleanHypercube::iter() order and its inverse (bh.rs:127-141), 2^num_vars entries each
void k_bh_order(Ctx&, size_t num_vars, uint32_t primitive, uint32_t* order, uint32_t* nth);
void k_one_hot_table(Ctx&, size_t n, size_t hot, Fr* out);
// Straight-line program over tables, constants and a small register file (the device counterpart of the
// reference's ExpressionRegistry calculations, util/expression/evaluator.rs:135-323): instruction i is
//   code[2i]   = op | dst << 4 | a_kind << 8 | b_kind << 10        code[2i+1] = a_idx | b_idx << 16
enum { PROG_ADD = 0, PROG_SUB = 1, PROG_MUL = 2, PROG_NEG = 3, PROG_MOV = 4 };
// (PROG_PAIR: table `idx` holds ONE entry per pair, the same at every evaluation point - the level of a factored eq table)
enum { PROG_REG = 0, PROG_ATOM = 1, PROG_CONST = 2, PROG_PAIR = 3 };
constexpr int PROG_MAX_REGS = 8;
struct ProgRound {
  const Fr* in[SC_MAX_TABLES];  // tables of 2 * size entries (already bound)
  uint32_t num_tables, num_instrs, num_regs, result_reg;
  const uint32_t* code;  // device
  const Fr* consts;      // device
};
// runtime-compiled form of a program (jit.cpp); nullptr = not compiled (disabled, too small, or compilation failed)
struct JitKernel;
bool jit_enabled(size_t num_vars);
// development / tests: the source the runtime compiler would be given (host code only)
std::string jit_debug_source(const uint32_t* code, size_t num_instrs, uint32_t num_regs, uint32_t result_reg, int degree);
const JitKernel* jit_sc_round(const Ctx&, const uint32_t* host_code, size_t num_instrs, uint32_t num_regs, uint32_t result_reg, int degree);
unsigned jit_blocks_per_cu(const JitKernel*);
void jit_launch(Ctx&, const JitKernel*, const ProgRound& pr, unsigned points, unsigned grid, size_t size, Fr* partials, const ScFinishArgs& fin);
// evals_host[0..points) = sum over pairs of program(tables at X), X = 1..points; `jit`: run the compiled form
void k_sc_round_prog(Ctx&, const ProgRound& pr, int points, size_t size, Fr* evals_host, const JitKernel* jit = nullptr);
// the linear part of a zero-check beside its eq-factored part (expr.cpp): out_host[0] = sum_i coeff_i sum_b t_i[2 b],
// out_host[1] = the same over the odd entries; queued in FRONT of the round's kernel, nobody waits for it alone
constexpr int LIN_MAX_TABLES = 8;
struct LinSums {
  const Fr* t[LIN_MAX_TABLES];
  Fr coeff[LIN_MAX_TABLES];
  uint32_t count;
};
void k_lin_sums(Ctx&, const LinSums& ls, size_t size, Fr* out_host);
enum { ROWS_ATOM_POLY = 0, ROWS_ATOM_IDENTITY = 1, ROWS_ATOM_LAGRANGE = 2 };
struct RowsAtom {
  const Fr* table;
  int32_t rot;
  uint32_t kind;
  uint64_t hot;  // Lagrange: the row where it is 1
};
struct RowsExpr {
  uint32_t num_terms, num_vars, primitive, x_inv;
  const Fr* coeff;       // device [num_terms]
  const uint32_t* off;   // device [num_terms + 1]
  const uint8_t* fac;    // device: atom ids
  const RowsAtom* atoms; // device
};
void k_expr_rows(Ctx&, const RowsExpr& e, size_t n, Fr* out);

// ------------------------------------------------------------------ HyperPlonk witness polys (kernels_plonk.hip)
// m[j] = #{i : input[i] == table[j]} on the LAST row j holding that value; false if an input is missing
bool k_lookup_m(Ctx&, const Fr* input, const Fr* table, size_t n, Fr* m_out);
// the same join with sizes of their own and the counts as the result: counts[r] = how many of the n inputs equal table row r,
// r < m (among equal rows the LAST takes every count; `counts` holds m + 1 words, the last is scratch); false: an input that
// is in no row.  Launch record "logup_m", n items
bool k_logup_multiplicities(Ctx&, const Fr* input, size_t n, const Fr* table, size_t m, uint32_t* counts);

// ------------------------------------------------------------------ LogUp-GKR (kernels_logup.hip)
constexpr int LOGUP_MAX = 8;  // LH_LOGUP_MAX_LOOKUPS and LH_LOGUP_MAX_WIDTH (include/lasso_hip.h)
// out[i] = sum_j pows[j] cols[j][i] over `width` (2 .. LOGUP_MAX) columns of n entries; pows[0] is one and is not applied
void k_logup_compress(Ctx&, const Fr* const* cols, const Fr* pows, size_t width, size_t n, Fr* out);
// the same sum over `width` (1 .. LOGUP_MAX) columns of which column j is a uint32_t column where u32[j] is set and an Fr
// column otherwise (at least one u32 column; width 1 widens it): a u32 entry costs 8 multiply-adds into the row's wide
// accumulator, which is reduced once.  pows[j] are the plain powers (Montgomery): the factor R of wide.cuh is applied here.
// Launch record "logup_compress_cols", algorithmic bytes sum_j (4 or 32) n + 32 n
void k_logup_compress_cols(Ctx&, const void* const* cols, const uint8_t* u32, const Fr* pows, size_t width, size_t n, Fr* out);
// The leaves of `count` fractions of 2^num_vars entries in ONE launch (blockIdx.y = the fraction), and with `up` the level
// above them (node i from the leaves i and i + half, fractional_sum_check.rs:62-85) in the same pass:
//   input side (m null):  q = gamma + c,  p == 1: the table `ones` shared by all fractions is filled, the level above is
//                         (q_l + q_r, q_l q_r) - no table of ones is read
//   table side:           p = -m (32-bit counts), q = gamma + c, the level above by the general formula
// Launch record "logup_leaves_up" (up) or "logup_leaves", count * 2^(num_vars - 1) items.
struct LogupLeaves {
  const Fr* c[LOGUP_MAX];
  const uint32_t* m[LOGUP_MAX];
  Fr* ones;
  Fr* p[LOGUP_MAX];  // table side
  Fr* q[LOGUP_MAX];
  Fr* p_up[LOGUP_MAX];
  Fr* q_up[LOGUP_MAX];
};
void k_logup_leaves(Ctx&, const LogupLeaves&, size_t count, size_t num_vars, bool table_side, bool up, const Fr& gamma);

// ------------------------------------------------------------------ read-write memory checking (kernels_memcheck.hip)
// The witness of a trace of 2^num_vars operations (addr, rv, wv: device u32 columns) over 2^mem_vars cells whose image is
// d_init (device; null: all zero): rt[i] = the time of the previous write to addr[i] (operation q writes at time q + 1; 0:
// none), fv[a] / ft[a] = the final value and time of cell a.  A stable sort of (addr, position) by the low mem_vars bits and one
// pass over the sorted positions; false (after ONE flag readback): an address >= 2^mem_vars or a read that does not return
// the last value written - the columns are then unspecified, but nothing is read or written out of bounds.
// Launch record "memcheck_trace", 2^num_vars items, algorithmic bytes 36 * 2^num_vars + 16 * 2^mem_vars
bool k_memcheck_trace(Ctx&, const uint32_t* addr, const uint32_t* rv, const uint32_t* wv, size_t num_vars, size_t mem_vars,
                      const uint32_t* d_init, uint32_t* rt, uint32_t* fv, uint32_t* ft);
// m[d] = #{i < n : i - rt[i] = d}, d < n, by wave-aggregated atomics.  Launch record "memcheck_m", n items, 12 n bytes
void k_memcheck_m(Ctx&, const uint32_t* rt, size_t n, uint32_t* m);
// The leaves of the four product trees in ONE launch, the side in blockIdx.y, h(a, v, t) = a gamma^2 + v gamma + t - tau:
//   side 0 (2^num_vars operations): col = addr, rv, rt, wv;        leaf = RS = h(addr, rv, rt), WS = h(addr, wv, i + 1)
//   side 1 (2^mem_vars cells):      col = init (null: 0), fv, ft;  leaf = Init = h(a, init, 0), Final = h(a, fv, ft)
// up[side] (both or neither of a side): the level above that side's leaves (node i = leaf[i] * leaf[i + half]) in the same pass.
// Launch record "memcheck_leaves", 2^num_vars + 2^mem_vars items.  `count` is filled by the launcher.
struct MemcheckLeaves {
  const uint32_t* col[2][4];
  Fr* leaf[2][2];
  Fr* up[2][2];
  size_t count[2];
};
void k_memcheck_leaves(Ctx&, const MemcheckLeaves&, size_t num_vars, size_t mem_vars, const Fr& gamma, const Fr& gamma2,
                       const Fr& tau);
// The leaves of the range check's two fractions over 2^num_vars entries in one launch, and with `up` the level above them:
//   fraction 0: p == 1 (`ones` is filled), q0 = delta + i - rt[i];   fraction 1: p1 = -m[i], q1 = delta + i
// Launch record "memcheck_range_leaves", 2^num_vars items
struct MemcheckRangeLeaves {
  const uint32_t *rt, *m;
  Fr *ones, *q0, *p1, *q1;
  Fr *p0_up, *q0_up, *p1_up, *q1_up;
};
void k_memcheck_range_leaves(Ctx&, const MemcheckRangeLeaves&, size_t num_vars, bool up, const Fr& delta);
// The replay of 2^num_vars operations (addr, store != 0, val: device u32 columns) over 2^mem_vars cells whose image is d_image
// (device; null: all zero): rv[i] = the word of the latest earlier store to addr[i], or the image's; wv[i] = store ? val : rv;
// fin[a] (null: not wanted) = the cell's word after the trace.  The stable sort of k_memcheck_trace, then an exclusive
// segmented scan over the sorted order in tiles of 2048 (three launches: tiles, the tiles' carries, the open operations).
// false (after ONE flag readback): an address >= 2^mem_vars - the outputs are then unspecified, nothing is out of bounds.
// Launch record "memcheck_replay", 2^num_vars items, algorithmic bytes 36 * 2^num_vars + (12 | 8 | 0) * 2^mem_vars
bool k_memcheck_replay(Ctx&, const uint32_t* addr, const uint32_t* store, const uint32_t* val, size_t num_vars, size_t mem_vars,
                       const uint32_t* d_image, uint32_t* rv, uint32_t* wv, uint32_t* fin);

// ------------------------------------------------------------------ Spark (kernels_spark.hip; spark.cpp, tests/spark_ref.py)
constexpr int SPARK_MAX_DIMS = 3;
// The memories of an opening in ONE launch: E[j][k] = T[j][dim[j][k]] for the `num_dims` dimensions (T[j]: 2^dim_vars field
// elements, a 32-byte gather by a u32 index - masked to dim_vars bits, so no index reads out of bounds), and the value
// v = sum_k val[k] prod_j E[j][k]: per-workgroup partial sums, then one workgroup adds them in a fixed order (the field
// sum is exact: the order does not matter for the bytes).  *out_value on the host; synchronises.
// Launch record "spark_e", n items, algorithmic bytes (32 + 68 num_dims) n
struct SparkE {
  const uint32_t* dim[SPARK_MAX_DIMS];
  const Fr* T[SPARK_MAX_DIMS];
  Fr* E[SPARK_MAX_DIMS];
  const Fr* val;
};
void k_spark_e(Ctx&, const SparkE&, size_t num_dims, size_t n, size_t dim_vars, Fr* out_value);
// The leaves of the 4 num_dims product trees in ONE launch, side and dimension in blockIdx.y (y = side * num_dims + j),
// h(a, v, t) = a gamma^2 + v gamma + t - tau:
//   side 0 (n entries): RS_j[k] = h(dim_j[k], E_j[k], read_ts_j[k]); WS_j = RS_j + 1 is written only where ws[j] is given
//   side 1 (2^dim_vars cells): Init_j[m] = h(m, T_j[m], 0), Final_j[m] = Init_j[m] + final_cts_j[m]
// up_n / up_l: the level above that side's leaves (node i = leaf[i] * leaf[i + half]) comes with them (rs_up, ws_up /
// init_up, fin_up: half the entries each).  Launch record "spark_leaves", num_dims (n + 2^dim_vars) items
struct SparkLeaves {
  const uint32_t *dim[SPARK_MAX_DIMS], *rts[SPARK_MAX_DIMS], *fcs[SPARK_MAX_DIMS];
  const Fr *E[SPARK_MAX_DIMS], *T[SPARK_MAX_DIMS];
  Fr *rs[SPARK_MAX_DIMS], *ws[SPARK_MAX_DIMS], *init[SPARK_MAX_DIMS], *fin[SPARK_MAX_DIMS];
  Fr *rs_up[SPARK_MAX_DIMS], *ws_up[SPARK_MAX_DIMS], *init_up[SPARK_MAX_DIMS], *fin_up[SPARK_MAX_DIMS];
};
void k_spark_leaves(Ctx&, const SparkLeaves&, size_t num_dims, size_t n, size_t dim_vars, bool up_n, bool up_l, const Fr& gamma,
                    const Fr& gamma2, const Fr& tau);

// ------------------------------------------------------------------ Spartan (kernels_spartan.hip; spartan.cpp, tests/spartan_ref.py)
// The keyed field sum of the three matrices in ONE launch set (the matrix in blockIdx.y):
//   out[m][s] = sum_{k: seg[m][k] = s} val[m][perm[m][k]] X[other[m][k]]      s < 2^dim_vars
// over the entry stream SORTED by seg (the R1CS key holds it: seg ascending, other and perm permuted along; perm[k] is the
// entry's position in the caller's order, where its value lives).  Entry-parallel: per-lane products, a segmented
// reduction by key over wave shuffles, the open ends of the 64-entry wave rows folded through LDS by one wave per tile, the
// open ends of the tiles by a short second kernel - a segment may span every tile; the cost follows n, not the longest
// segment.  Indices are masked to dim_vars bits and perm to n: nothing is read or written out of bounds whatever the
// columns hold.  out is zeroed first: segments without entries are zero.  carry_k / carry_v: the launcher's (arena).
// Launch record "spartan_spmv", 3 n items and products, algorithmic bytes 3 (76 n + 32 * 2^dim_vars)
constexpr int SPMV_TILE = 2048;  // entries per workgroup: THE tile (at most 4096: tests/test_gpu_spartan_spmv.py rests on that)
struct SpartanSpmv {
  const uint32_t *seg[3], *other[3], *perm[3];
  const Fr* val[3];
  const Fr* X;
  Fr* out[3];
  uint32_t* carry_k;
  Fr* carry_v;
};
void k_spartan_spmv(Ctx&, const SpartanSpmv&, size_t n, size_t dim_vars);
// the number of rows i < rows with az[i] bz[i] != cz[i]; synchronises.  Launch record "spartan_unsatisfied"
size_t k_spartan_unsatisfied(Ctx&, const Fr* az, const Fr* bz, const Fr* cz, size_t rows);

// ------------------------------------------------------------------ Nova folding (kernels_nova.hip; nova.cpp, tests/nova_ref.py)
// spartan_spmv with TWO right-hand sides in one pass over the sorted stream: out1[m][s] = sum val X1[other], out2[m][s] = sum
// val X2[other].  Key, other index, position and the value are loaded once for both; the same tile, scan, store-or-carry and
// fold structure with carry items of a key and two sums.  X1 and X2 may be one vector.  Both outs are zeroed first.
// Launch record "nova_spmv2", 3 n items, 6 n products, algorithmic bytes 3 (108 n + 64 * 2^dim_vars)
struct NovaSpmv2 {
  const uint32_t *seg[3], *other[3], *perm[3];
  const Fr* val[3];
  const Fr *X1, *X2;
  Fr *out1[3], *out2[3];
  uint32_t* carry_k;
  Fr *carry_v1, *carry_v2;
};
void k_nova_spmv2(Ctx&, const NovaSpmv2&, size_t n, size_t dim_vars);
// t[i] = mz1[0][i] mz2[1][i] + mz2[0][i] mz1[1][i] - u1 mz2[2][i] - u2 mz1[2][i], and bad[k] = the number of rows at which
// input k fails mz[0] mz[1] = u mz[2] + e (e1 / e2 null: zero); synchronises.  Launch record "nova_cross_term"
struct NovaCross {
  const Fr *mz1[3], *mz2[3];
  const Fr *e1, *e2;
  Fr* t;
};
void k_nova_cross_term(Ctx&, const NovaCross&, const Fr& u1, const Fr& u2, size_t rows, size_t bad[2]);
// the count alone, of one input; synchronises.  Launch record "nova_unsatisfied"
size_t k_nova_unsatisfied(Ctx&, const Fr* az, const Fr* bz, const Fr* cz, const Fr& u, const Fr* e, size_t rows);
// w_out = w1 + r w2 over `half` entries and e_out = e1 + r t + r2 e2 over `rows` in ONE launch (e1, e2 null: zero); the outputs
// may be the inputs.  Launch record "nova_fold"
void k_nova_fold(Ctx&, const Fr* w1, const Fr* w2, Fr* w_out, const Fr* e1, const Fr* t, const Fr* e2, Fr* e_out, const Fr& r,
                 const Fr& r2, size_t half, size_t rows);

void k_lookup_h(Ctx&, const Fr* input, const Fr* table, const Fr* m, const Fr& gamma, size_t n, Fr* h);
void k_permutation_z(Ctx&, const Fr* const* values, const Fr* const* perms, size_t num_perm, size_t num_chunks,
                     size_t num_vars, const Fr& beta, const Fr& gamma, const uint32_t* d_order, const uint32_t* d_nth,
                     Fr* const* z_out);
void k_permutation_products(Ctx&, const Fr* const* values, const Fr* const* perms, size_t num_perm, size_t num_chunks,
                            size_t num_vars, const Fr& beta, const Fr& gamma, size_t n, size_t sj, size_t srho, size_t srank,
                            Fr* const* prod_out);
void k_permutation_z_from_products(Ctx&, const Fr* const* prods, size_t num_chunks, size_t num_vars, const uint32_t* d_order,
                                   const uint32_t* d_nth, Fr* const* z_out, size_t sj, size_t srho, size_t srank);
void k_scatter_rows(Ctx&, const uint32_t* d_rows, const Fr* d_vals, size_t count, size_t n, Fr* table);

// ------------------------------------------------------------------ Zeromorph / univariate KZG (kernels_zm.hip)
void k_powers(Ctx&, const Fr& s, size_t n, Fr* out);  // out[i] = s^i
// q: quotients flat (q_k at offset 2^k - 1); ypow / q_scalars: host arrays of num_vars elements
void k_zm_qhat(Ctx&, const Fr* q, size_t num_vars, const Fr* ypow, Fr* q_hat);
void k_zm_combine(Ctx&, const Fr* poly, const Fr* q_hat, const Fr* q, size_t num_vars, const Fr& z,
                  const Fr* q_scalars, Fr* f);
// out[i] = sum_{j >= i} f_j x^(j - i): out[1..] is the quotient of f by (X - x), out[0] = f(x)
void k_suffix_horner(Ctx&, const Fr* f, size_t n, const Fr& x, Fr* out);

// ------------------------------------------------------------------ Gemini / batched univariate KZG (kernels_gemini.hip)
constexpr int GM_MAX_VARS = 32;
constexpr size_t GM_TAIL_IN = 1024;   // folds of at most this many input coefficients run inside one workgroup's LDS
constexpr size_t GM_CHUNK = 64;       // positions per thread of the batched suffix Horner
constexpr uint32_t GM_MAX_STRIDE = 2;
// folds[off_i ..] = fs[i], i = 1 .. num_vars - 1 (2^(num_vars - i) coefficients; off_1 = 0, off_{i+1} = off_i + 2^(num_vars - i)):
// fs[i][j] = fs[i-1][2j] + xs[i-1] (fs[i-1][2j+1] - fs[i-1][2j]), fs[0] = poly; xs: host array of num_vars - 1 elements
void k_gm_fold_chain(Ctx&, const Fr* poly, size_t num_vars, const Fr* xs, Fr* folds);
struct GmEvalSeg {
  const Fr* f;
  size_t len;  // even
  Fr x2;
};
// out (host) [2 s], [2 s + 1] = sum_j f_s[2j] x2_s^j, sum_j f_s[2j+1] x2_s^j; synchronises
void k_gm_eval_even_odd(Ctx&, const GmEvalSeg* segs, size_t count, Fr* out);
struct GmHornerSeg {
  const Fr* f;
  Fr* out;  // len entries, may not alias f
  size_t len;
  uint32_t stride;  // 1 or 2
  Fr x;
};
// out[i] = f[i] + x out[i + stride] (zero beyond len): out[stride..] = the quotient of f by X^stride - x, out[..stride] the remainder
void k_gm_suffix_horner(Ctx&, const GmHornerSeg* segs, size_t count);
struct GmTerm {
  const Fr* p;
  size_t len;
  Fr w;
};
// out[j] = sum_{k : j < len_k} w_k p_k[j], j < n (out aliases no term)
void k_gm_combine(Ctx&, const GmTerm* terms, size_t count, size_t n, Fr* out);

// ------------------------------------------------------------------ multilinear IPA (kernels_ipa.hip)
// out[j] = g[first + j] of the library's hash-to-point, j < n; queued on the stream
void k_ipa_generators(Ctx&, size_t first, size_t n, G1Affine* out);
// the base fold: out[j] = a[j] + s b[j], affine (identity = (0,0)); out may be a (not b).  Temporary storage from the arena.
void k_g1_axpy(Ctx&, const G1Affine* a, const G1Affine* b, size_t n, const Fr& s, G1Affine* out);
constexpr size_t IPA_CROSS_BLOCKS = 1024;
// d_out[0] = <coeffs[mid..2 mid), zs[..mid)>, d_out[1] = <coeffs[..mid), zs[mid..2 mid)> (DEVICE, queued on the stream);
// d_partials: 2 IPA_CROSS_BLOCKS elements of scratch
void k_ipa_cross(Ctx&, const Fr* coeffs, const Fr* zs, size_t mid, Fr* d_partials, Fr* d_out);
// out_c[i] = coeffs[i] + xi_inv coeffs[mid + i], out_z[i] = zs[i] + xi zs[mid + i], i < mid (in place allowed)
void k_ipa_fold_fr(Ctx&, const Fr* coeffs, const Fr* zs, size_t mid, const Fr& xi_inv, const Fr& xi, Fr* out_c, Fr* out_z);

// Hyrax's row combination (fix_last_vars, hyrax.rs:243): out[c] = sum_r w[r] poly[r row_len + c], c < row_len, r < rows;
// w on the device; temporary storage from the arena
void k_hyrax_combine(Ctx&, const Fr* poly, const Fr* w, size_t rows, size_t row_len, Fr* out);

// ------------------------------------------------------------------ Hyrax's row commitments (kernels_hyrax.hip)
// out_host[r] = sum_{c < row_len} s[r row_len + c] bases[c], r < ceil(n / row_len): the rows of a flat array of n scalars, Fr
// (Montgomery) or u32 with every value < 2^bits (bits in 1..32); a partial last row is padded with zeros; affine, the identity
// as (0, 0).  win_table: the window table of `bases` (k_msm_window_table over row_len points, cbits = 8, W >= the windows the
// column needs: g1_rows_msm_windows) or null - then a temporary one is built in the arena.  Synchronises.
void k_g1_rows_msm(Ctx&, const void* scalars, bool u32, uint32_t bits, size_t n, size_t row_len, const G1Affine* bases,
                   const G1Affine* win_table, uint32_t cbits, uint32_t W, G1Affine* out_host);
// the same for a batch of columns over the same bases in one launch set: column i gives rows_per_col points at
// out_host[i rows_per_col ..]; the rows beyond its n entries launch no work and come out as identities
struct RowsMsmCol {
  const void* scalars;
  bool u32;
  uint32_t bits;
  size_t n;
};
void k_g1_rows_msm_batch(Ctx&, const RowsMsmCol* cols, size_t num_cols, size_t rows_per_col, size_t row_len, const G1Affine* bases,
                         const G1Affine* win_table, uint32_t cbits, uint32_t W, G1Affine* out_host);
uint32_t g1_rows_msm_windows(bool u32, uint32_t bits);  // 8-bit windows of a column: 32 for Fr, ceil(bits / 8) for u32
size_t g1_rows_msm_segment(bool u32);                   // columns of a row one workgroup takes: 256 for Fr, 2048 for u32

// ------------------------------------------------------------------ radix sort (sort.hip)
// stable sort of (u32 key, u32 value) pairs by the low `bits` bits of the key; inputs are preserved
struct SortSlab {
  const uint32_t* keys_in;
  uint32_t* keys_out;
  const uint32_t* vals_in;
  uint32_t* vals_out;
  size_t n;
  unsigned bits;
  unsigned first_bit = 0;
};
// (vals_in == nullptr: the values are the positions 0 .. n - 1; the sort is by the key bits [first_bit, first_bit + bits),
// which must end inside the key: LH_ERR_ARG otherwise; `bits` above the key width count as the key width)
void sort_pairs_u32(Ctx&, const uint32_t* keys_in, uint32_t* keys_out, const uint32_t* vals_in, uint32_t* vals_out, size_t n,
                    unsigned bits, unsigned first_bit = 0);
// `count` independent sorts as ONE launch set per radix pass (temporary storage from the arena: the caller's ArenaScope)
void sort_pairs_u32_batched(Ctx&, const SortSlab* slabs, size_t count);
// (by the low `bits` bits of a u64 key; every caller today passes 64)
void sort_pairs_u64(Ctx&, const uint64_t* keys_in, uint64_t* keys_out, const uint32_t* vals_in, uint32_t* vals_out, size_t n,
                    unsigned bits);
// the plan of one slab (host only; lh_debug_sort_plan): passes, the digit width of every pass (rb[passes .. 8) = 0) and the
// arena bytes the sort takes
void sort_plan(size_t n, unsigned bits, size_t key_bytes, unsigned* passes, unsigned rb[8], size_t* temp_bytes);

// ------------------------------------------------------------------ MSM (msm.hip)
struct MsmJob {
  const void* scalars;  // Fr (Montgomery) or u32
  bool scalars_u32;
  const G1Affine* bases;
  size_t n;
  // Optional: this column is a table of another column of the batch, scalars[i] = table[parent.scalars[i]] (Lasso's
  // E = T[dim]).  When the parent ends up with ONE window whose bucket index is the parent's value, this job's buckets
  // are sums of the PARENT'S buckets (S_v = sum of B_d over T[d] = v) and no pass over its n points is made: 2^in_bits
  // bucket additions instead of n point additions.  Otherwise the job runs as an ordinary u32 column.
  int derived_parent = -1;             // index of the parent job in the same batch
  const uint32_t* d_table = nullptr;   // device: T[d], d < 2^table_in_bits; T[0] must be 0
  const uint32_t* d_order = nullptr;   // device: 0 .. 2^table_in_bits - 1 sorted by T (any order inside equal T)
  uint32_t table_in_bits = 0, table_out_bits = 0;
  // Optional (u32 columns): the column's values in ascending order and the positions they came from (Lasso's access
  // counters sort every dim column anyway).  A job that ends up with one window per (job, window) slab takes its sorted
  // entry stream from these instead of emitting and sorting it again.
  const uint32_t* sorted_scalars = nullptr;
  const uint32_t* sorted_index = nullptr;
  // Optional (u32 columns): TWO small-valued columns over the same bases packed into one, scalars[i] = s1[i] | s2[i] <<
  // pack_shift (4 <= pack_shift, at most MSM_PACK_MAX_BITS significant bits together).  One pass over the points fills one
  // bucket set indexed by the packed value; the reduction weighs it twice: out[j] = sum s1[i] B_i, *out_second = sum s2[i] B_i.
  uint32_t pack_shift = 0;
  G1Affine* out_second = nullptr;  // host
  // Optional: every scalar < 2^known_bits, promised by the caller (0: measured by a pass over the scalars - a column
  // that happens to be narrower then gets fewer windows; a promise that is too small loses the upper bits)
  uint32_t known_bits = 0;
  // Optional (Fr columns): the window table of `bases` (k_msm_window_table: entry w * n + i = 2^(win_table_c w) * bases[i],
  // w < win_table_W).  A column that needs 2 .. win_table_W windows of win_table_c bits then files all of them into one
  // bucket set (one bucket reduction, no doublings) - same sum, W-fold fewer buckets.
  const G1Affine* win_table = nullptr;
  uint32_t win_table_c = 0, win_table_W = 0;
};
constexpr uint32_t MSM_PACK_MAX_BITS = 20;
// two columns share a pass only while the pass saved (one mixed addition per point) outweighs the bucket set it adds to the
// reduction (2^bits buckets at ~3.5 full additions each): from 8 points per bucket on.  (The single-GPU sizes that pack are
// far above it; a rank's shard of a level - 2^20 points against 2^20 buckets at 8 ranks - is not.)
constexpr size_t MSM_PACK_MIN_POINTS_PER_BUCKET = 8;
Ctx& ctx_helper(Ctx&);            // the ctx's helper ctx (created on first use, destroyed with the ctx)
void open_precommit_cancel(Ctx&);  // waits for a running precommit and drops it (open_columns.cpp)
void open_precommit_release(Ctx&);  // a staged precommit's second stage may run from here on the ctx's stream (no-op otherwise)
uint32_t msm_window_bits(size_t n);  // window width msm_batch picks for a full-width (254-bit) column of n points
void k_msm_window_table(Ctx&, const G1Affine* bases, size_t n, uint32_t cbits, uint32_t W, G1Affine* out);
// Runs all jobs as one batched Pippenger; out[j] is the affine sum (identity = (0,0)).
// `overlap` (optional): host work that needs none of this batch's results - run once, after the batch's kernels are
// queued and before the host waits for the window sums (it overlaps the device's work instead of following it)
// Returns whether the host waited for the ctx's stream on the way (false only for a batch without a single entry and with every
// width promised: then nothing queued before the call is known to have run).
// `acc_queued` (optional): called once, on the calling thread, right behind the batch's last bucket-accumulation launch (a
// batch without entries: before the call returns) - `on_aux`: a second half's accumulation went to the ctx's aux stream.
// An event recorded there on the stream(s) marks the end of the batch's ALU-bound stretch: only latency-bound tails follow
bool msm_batch(Ctx&, const MsmJob* jobs, size_t num_jobs, G1Affine* out_host, const std::function<void()>* overlap = nullptr,
               const std::function<void(bool on_aux)>* acc_queued = nullptr);
// msm_batch in two calls, for a caller that wants the challenge-free front of a batch queued early and its ALU-bound part
// held back (open_columns.cpp): msm_prepare plans the batch, allocates its workspace from the ctx's arena and queues digits
// and sort - the sorted entry stream is then in the arena -; msm_run queues accumulation, continuation levels, reduction and
// window sums, waits and combines on the host.  The caller's ArenaScope spans both calls, nothing else uses the ctx in
// between, and `jobs` are the same array.  msm_batch is msm_prepare followed by msm_run.
struct MsmPrepared;
struct MsmPreparedDelete {
  void operator()(MsmPrepared*) const;
};
typedef std::unique_ptr<MsmPrepared, MsmPreparedDelete> MsmPreparedPtr;
MsmPreparedPtr msm_prepare(Ctx&, const MsmJob* jobs, size_t num_jobs);
bool msm_run(Ctx&, MsmPrepared&, const MsmJob* jobs, size_t num_jobs, G1Affine* out_host);
// the planning half alone (host only; lh_debug_msm_plan): the shape msm_prepare arrives at for jobs of these sizes, widths
// (bits[j] significant bits, promised) and kinds, as SHAPE_WORDS numbers per sub-batch -> the number of sub-batches
constexpr size_t MSM_SHAPE_WORDS = 12;
size_t msm_plan_shape(Ctx&, const MsmJob* jobs, size_t num_jobs, bool via_prepare, uint64_t* out /* [2 * MSM_SHAPE_WORDS] */);
// out[i] = scalars[i] * G (fixed-base), normalised to affine; all on device
void k_fixed_base_mul_g(Ctx&, const Fr* scalars, size_t n, G1Affine* out);

}  // namespace lh
