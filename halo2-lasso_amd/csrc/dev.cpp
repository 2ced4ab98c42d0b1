// Device context and workspace arena.
#include <string.h>
#include <stdlib.h>
#include <ctype.h>
#include <errno.h>
#include <sched.h>
#include <atomic>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <functional>
#include <memory>
#include <emmintrin.h>
#include <hip/hip_ext.h>
#include <vector>
#include <chrono>
#include "host.hpp"  // spark_free_all, spartan_free_all (Ctx::~Ctx)

namespace lh {

static thread_local std::string g_last_error;
void set_last_error(const char* msg) { g_last_error = msg ? msg : ""; }
const char* get_last_error() { return g_last_error.c_str(); }

// ------------------------------------------------------------------ owners (owned.hpp)
namespace {
enum { LIVE_DEV, LIVE_PINNED, LIVE_EVENT, LIVE_STREAM };
std::atomic<uint64_t> g_live[4];
std::atomic<int64_t> g_fail_after{-1};
// ahead of every acquisition: false when this one is the injected failure
bool acquire_allowed() {
  return g_fail_after.load(std::memory_order_relaxed) < 0 || g_fail_after.fetch_sub(1, std::memory_order_relaxed) != 0;
}
void acquire_gate() {
  if (!acquire_allowed()) throw Error(LH_ERR_DEVICE, "injected acquisition failure (lh_debug_fail_acquire_after)");
}
void live(int kind, int by) { g_live[kind].fetch_add((uint64_t)(int64_t)by, std::memory_order_relaxed); }
}  // namespace
void owned_live(uint64_t out[4]) {
  for (int k = 0; k < 4; k++) out[k] = g_live[k].load(std::memory_order_relaxed);
}
void owned_fail_acquire_after(int64_t n) { g_fail_after.store(n < 0 ? -1 : n, std::memory_order_relaxed); }

OnDevice::OnDevice(int device, bool nothrow) {
  if (device < 0) return;
  if (hipGetDevice(&prev) != hipSuccess) prev = -1;
  if (prev == device) return;
  const hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) switched = true;
  else if (!nothrow) throw Error(LH_ERR_DEVICE, std::string("hipSetDevice(device): ") + hipGetErrorString(e));
}
OnDevice::~OnDevice() {
  if (switched && prev >= 0) (void)hipSetDevice(prev);
}

bool DevMem::try_alloc(size_t bytes) {
  reset();
  if (!acquire_allowed() || hipGetDevice(&device_) != hipSuccess || hipMalloc(&p_, bytes) != hipSuccess) {
    p_ = nullptr;
    return false;
  }
  bytes_ = bytes;
  live(LIVE_DEV, 1);
  return true;
}
void DevMem::alloc(size_t bytes) {
  reset();
  acquire_gate();
  LH_HIP(hipGetDevice(&device_));
  LH_HIP(hipMalloc(&p_, bytes));
  bytes_ = bytes;
  live(LIVE_DEV, 1);
}
void DevMem::forget() {
  p_ = nullptr, bytes_ = 0;
  live(LIVE_DEV, -1);
}
void DevMem::reset() {
  if (!p_) return;
  OnDevice on(device_, true);
  (void)hipFree(p_);
  forget();
}

void PinnedMem::alloc(size_t bytes) {
  reset();
  acquire_gate();
  LH_HIP(hipHostMalloc(&p_, bytes, flags_));
  bytes_ = bytes;
  live(LIVE_PINNED, 1);
}
void PinnedMem::reset() {
  if (!p_) return;
  (void)hipHostFree(p_);
  p_ = nullptr, bytes_ = 0;
  live(LIVE_PINNED, -1);
}

void Event::create() {
  acquire_gate();
  LH_HIP(hipEventCreateWithFlags(&ev_, flags_));
  live(LIVE_EVENT, 1);
}
void Event::reset() {
  if (!ev_) return;
  (void)hipEventDestroy(ev_);
  ev_ = nullptr;
  live(LIVE_EVENT, -1);
}

void Stream::create(unsigned flags) {
  reset();
  acquire_gate();
  LH_HIP(hipStreamCreateWithFlags(&s_, flags));
  live(LIVE_STREAM, 1);
}
void Stream::create(unsigned flags, int priority) {
  reset();
  acquire_gate();
  LH_HIP(hipStreamCreateWithPriority(&s_, flags, priority));
  live(LIVE_STREAM, 1);
}
void Stream::reset() {
  if (!s_) return;
  (void)hipStreamDestroy(s_);
  s_ = nullptr;
  live(LIVE_STREAM, -1);
}


void* Arena::alloc(size_t bytes) {
  bytes = (bytes + 255) & ~(size_t)255;
  if (bytes == 0) bytes = 256;
  return alloc_raw(bytes);
}
void* Arena::alloc_raw(size_t bytes) {
  while (true) {
    if (!blocks_.empty()) {
      Block& b = blocks_[cur_];
      if (b.used + bytes <= b.size) {
        void* p = b.mem.as<char>() + b.used;
        b.used += bytes;
        size_t tot = 0;
        for (size_t i = 0; i <= cur_; i++) tot += blocks_[i].used;
        if (tot > high_) high_ = tot;
        return p;
      }
      if (cur_ + 1 < blocks_.size()) {
        cur_++;
        blocks_[cur_].used = 0;
        continue;
      }
    }
    size_t want = blocks_.empty() ? ((size_t)64 << 20) : blocks_.back().size * 2;
    if (want < bytes) want = bytes;
    blocks_.push_back(Block{DevMem(want), want, 0});
    cur_ = blocks_.size() - 1;
  }
}

void Arena::release(Mark m) {
  if (blocks_.empty()) return;
  for (size_t i = m.block + 1; i < blocks_.size(); i++) blocks_[i].used = 0;
  cur_ = m.block;
  blocks_[cur_].used = m.used;
}

Ctx::Ctx(int device_id) : device(device_id) {
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0)
    throw Error(LH_ERR_DEVICE, "no HIP device available (this library has no CPU fallback)");
  LH_REQUIRE(device_id >= 0 && device_id < count, LH_ERR_DEVICE, "device id out of range");
  LH_HIP(hipSetDevice(device_id));
  stream.create(hipStreamNonBlocking);
  hipDeviceProp_t prop;
  LH_HIP(hipGetDeviceProperties(&prop, device_id));
  num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  int khz = 0;
  if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device_id) == hipSuccess && khz > 0) wall_clock_khz = khz;
  pin(65536);
  host_trace_on = knob(Knob::HOST_TRACE) != 0;
  // line 0: device -> host sequence flag; lines 1-2: host -> device mailbox of the resident sum-check tail
  flag.alloc(256);
  memset(flag.get(), 0, 256);
  ticket.alloc(256);  // word 0: ticket, word 8: device flag, words 32..47: the tail's relay chunks
  LH_HIP(hipMemset(ticket, 0, 256));
  fin_lanes.alloc((size_t)FIN_LANE_SUMS * 64);
  LH_HIP(hipMemset(fin_lanes, 0, (size_t)FIN_LANE_SUMS * 64));
}

Ctx::~Ctx() {
  try {
    open_precommit_cancel(*this);
  } catch (...) {
  }
  spartan_free_all(*this);  // (R1CS keys nobody freed: before the polynomials they own)
  spark_free_all(*this);    // (committed sparse polynomials nobody freed: their device memory goes with the ctx)
  helper.reset();
  worker.reset();  // (joins; after the precommit it may still be running was cancelled above)
  if (aux_stream) (void)hipStreamSynchronize(aux_stream);
  if (stream) (void)hipStreamSynchronize(stream);
  try {
    comm_detach(*this);
  } catch (...) {
  }
}

Ctx& ctx_helper(Ctx& c) {
  if (!c.helper) {
    c.helper.reset(new Ctx(c.device));
    c.helper->is_helper = true;
  }
  return *c.helper;
}

uint64_t* Ctx::lanes_host_block() {
  if (!lanes_host) {
    lanes_host.alloc(128 * sizeof(uint64_t));
    memset(lanes_host.get(), 0, 128 * sizeof(uint64_t));
  }
  return lanes_host;
}

void Ctx::opt_in_lds(const void* fn, int bytes) {
  for (const void* f : lds_opted)
    if (f == fn) return;
  LH_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
  lds_opted.push_back(fn);
}

static const struct {
  const char* name;
  int64_t Options::*field;
  int64_t lo, hi;  // accepted range (shift counts stay below 64, lengths are never negative)
} OPTION_TABLE[] = {
    {"open_small_min_vars", &Options::open_small_min_vars, 0, 64}, {"open_small_depth", &Options::open_small_depth, 0, 2},
    {"sc_eq_factoring", &Options::sc_eq_factoring, 0, 1},          {"lasso_pack_ts", &Options::lasso_pack_ts, 0, 1},
    {"sc_tail", &Options::sc_tail, 0, 1},                          {"sc_tail_max_len", &Options::sc_tail_max_len, 0, (int64_t)1 << 20},
    {"shard_exchange_log", &Options::shard_exchange_log, 0, 40},   {"msm_window_tables", &Options::msm_window_tables, 0, 40},
    {"open_precommit", &Options::open_precommit, 0, 64},           {"gkr_resident", &Options::gkr_resident, 0, 1},
    {"open_precommit_stages", &Options::open_precommit_stages, 0, 1},
    {"sc_pp_fold", &Options::sc_pp_fold, 0, 2},                    {"msm_half_batches", &Options::msm_half_batches, 0, 1},
    {"comm_round", &Options::comm_round, 0, 2},                    {"hyrax_rows", &Options::hyrax_rows, 0, 1},
    {"brakedown_batch_commit", &Options::brakedown_batch_commit, 0, 1}, {"brakedown_staged_open", &Options::brakedown_staged_open, 0, 1},
    {"brakedown_u32_gather", &Options::brakedown_u32_gather, 0, 1}, {"logup_fused_leaves", &Options::logup_fused_leaves, 0, 1},
};

int64_t* Options::find(const char* name) {
  if (!name) return nullptr;
  for (const auto& o : OPTION_TABLE)
    if (strcmp(o.name, name) == 0) return &(this->*o.field);
  return nullptr;
}
bool Options::in_range(const char* name, int64_t value) {
  if (!name) return false;
  for (const auto& o : OPTION_TABLE)
    if (strcmp(o.name, name) == 0) return value >= o.lo && value <= o.hi;
  return false;
}

// The one parse of an environment value, options and knobs: false when `name` is unset, empty, not a number (an integer
// unless `real`) or outside [lo, hi] - ignored, loudly (nobody is there to take an error; with `said`: once).
static bool env_number(const char* name, bool real, double lo, double hi, double& out, std::atomic<bool>* said = nullptr) {
  const char* e = getenv(name);
  if (!e || !*e) return false;
  char* end = nullptr;
  errno = 0;
  const double v = real ? strtod(e, &end) : (double)strtoll(e, &end, 10);
  if (end != e && *end == 0 && errno == 0 && v >= lo && v <= hi) {
    out = v;
    return true;
  }
  if (!said || !said->exchange(true))
    fprintf(stderr, "[lasso-hip] %s=%s is outside [%lld, %lld]: ignored\n", name, e, (long long)lo, (long long)hi);
  return false;
}

Options::Options() {
  for (const auto& o : OPTION_TABLE) {
    std::string env = "LH_";
    for (const char* p = o.name; *p; p++) env.push_back((char)toupper((unsigned char)*p));
    double v;
    if (!env_number(env.c_str(), false, (double)o.lo, (double)o.hi, v)) continue;
    this->*o.field = (int64_t)v;
    if (o.field == &Options::open_small_min_vars) open_small_min_vars_forced = true;
  }
}

// (row i is Knob i: tests/test_knobs.py holds the two lists to the same order)
enum KnobKind { INT, REAL, WORD, PATH };
static constexpr struct KnobRow {
  const char* env;
  KnobKind kind;
  double dflt, lo, hi;  // (a switch is an INT in [0, 1]; WORD: 1 when the value is `word`)
  bool live;            // read at every use (tests change it within a process), not once
  const char* word;
} KNOB_TABLE[] = {
    // thresholds between code paths
    {"LH_SC_TAIL_G", INT, 0, 0, 1024},                 // workgroups of the resident tail (0: by size)
    {"LH_MSM_C_OFF", INT, 4, -32, 32},                 // MSM window: floor(log2 n) - this, at most LH_MSM_C_MAX
    {"LH_MSM_C_MAX", INT, 17, 1, 31},
    {"LH_MSM_K2", INT, 4, 2, 64},                      // fan-in of the linear continuation levels
    {"LH_MSM_SEG", INT, 0, 0, 256},                    // buckets per reduction segment (0: by size)
    {"LH_MSM_SLAB_LOG", INT, 16, 0, 31},               // jobs of >= 2^this points: sorted slab by slab
    {"LH_MSM_TREE_MAX", INT, 262144, 0, 1 << 30},      // continuation lists up to this: trees (0: never)
    {"LH_MSM_QUAD_MAX", INT, 262144, 0, 1 << 30},      // lists / segments up to this: a quad of lanes each (0: never)
    {"LH_MSM_TWO_LEVEL", INT, 1, 0, 1},                // two-level bucket reduction
    {"LH_MSM_HALF_MIN_LOG", INT, 24, 0, 63},           // batches of >= 2^this entries: two halves
    {"LH_MSM_HALF_COVER", INT, 12, 0, 1 << 20},        // second-half entries per first-half bucket
    {"LH_EXPR_MONOMIALS", INT, 0, 0, 1},               // sum of monomials, not the register program
    {"LH_EXPR_JIT_MIN_VARS", INT, 16, 0, 64},          // smallest sum-check with a compiled kernel
    {"LH_EXPR_EF_MIN_VARS", INT, 14, 2, 64},           // smallest eq-factored expression sum-check
    // A/B switches of round 6's routes (the bytes never depend on them)
    {"LH_FIN_LANES_MIN_BYTES", REAL, 0, -1, 1e18},     // -1: no launch hands over in lanes
    {"LH_SC_U32", INT, 1, 0, 1}, {"LH_OPEN_U32_ROUNDS", INT, 1, 0, 1}, {"LH_OPEN_FOLD_COLS", INT, 1, 0, 1},
    {"LH_OPEN_SHARE_SUMS", INT, 1, 0, 1, true},        // the opening takes the evaluation passes' quad sums (live: tests flip it)
    // 1: a product g whose value fits 32 bits (less_than / equal tables) gets a 32-bit output column (lasso.cpp; off: its
    // gain at 2^20 lookups stayed inside the spread; live: tests flip it)
    {"LH_LASSO_PRODUCT_U32", INT, 0, 0, 1, true},
    // operation
    {"LH_HOST_THREADS", INT, 48, 0, 4096},             // host pool threads, the caller's included
    {"LH_JIT_CACHE", INT, 1, 0, 1}, {"LH_JIT_CACHE_DIR", PATH, 0, 0, 0},
    {"LH_EXPR_JIT", INT, 1, 0, 1},                     // 0: always interpret
    {"LH_SC_TAIL_TIMEOUT_MS", REAL, 2000, 0, 1e7, true}, {"LH_GKR_START_TIMEOUT_MS", REAL, 25, 0, 1e7, true},
    {"LH_COMM_WAIT_TIMEOUT_MS", INT, 30000, 1, 1e9}, {"LH_COMM_A2A", WORD, 0, 0, 1, false, "allgather"},
    {"LH_COMM_PROBE", INT, 1, 0, 1},
    // diagnostics (stderr)
    {"LH_HOST_TRACE", INT, 0, 0, 1, true}, {"LH_SC_TAIL_TRACE", INT, 0, 0, 1}, {"LH_GKR_TRACE", INT, 0, 0, 1},
    {"LH_SC_DEBUG", INT, 0, 0, 1}, {"LH_MSM_DEBUG", INT, 0, 0, 1}, {"LH_HP_DEBUG", INT, 0, 0, 1}, {"LH_COMM_DEBUG", INT, 0, 0, 1},
    {"LH_OPEN_SMALL_CHECK", INT, 0, 0, 1},
    // test hooks
    {"LH_COMM_A2A_SELF", INT, 0, 0, 1}, {"LH_COMM_PROBE_FAIL", INT, 0, 0, 1}, {"LH_SHARDED_COUNTERS_MIN_R", INT, 2, 1, 1 << 20},
    // a Lasso prove's precommit (open_columns.cpp): 1 = the trees' callback does nothing, so a staged precommit is released only
    // when the opening takes it (and a single-stage one never starts); 2 = the same, and the opening cancels it and commits
    // the column-wise levels itself (live: tests flip it)
    {"LH_TEST_PRECOMMIT_GATE", INT, 0, 0, 2, true},
};
static_assert(sizeof(KNOB_TABLE) / sizeof(KNOB_TABLE[0]) == (size_t)Knob::COUNT, "KNOB_TABLE: one row per Knob");

static double knob_read(const KnobRow& r, std::atomic<bool>* said) {
  double v = r.dflt;
  if (r.kind != WORD) {
    env_number(r.env, r.kind == REAL, r.lo, r.hi, v, said);
  } else if (const char* e = getenv(r.env)) {
    if (strcmp(e, r.word) == 0) v = 1;
    else if (*e && (!said || !said->exchange(true))) fprintf(stderr, "[lasso-hip] %s=%s is outside [%s]: ignored\n", r.env, e, r.word);
  }
  return v;
}

double knob(Knob k) {
  constexpr size_t N = (size_t)Knob::COUNT;
  static const std::vector<double> once = [] {
    std::vector<double> v(N);
    for (size_t i = 0; i < N; i++)
      if (!KNOB_TABLE[i].live && KNOB_TABLE[i].kind != PATH) v[i] = knob_read(KNOB_TABLE[i], nullptr);
    return v;
  }();
  static std::atomic<bool> said[N];  // (a live knob's bad value is reported once, too)
  const KnobRow& r = KNOB_TABLE[(size_t)k];
  return r.live ? knob_read(r, &said[(size_t)k]) : once[(size_t)k];
}

const char* knob_text(Knob k) {
  const char* e = KNOB_TABLE[(size_t)k].kind == PATH ? getenv(KNOB_TABLE[(size_t)k].env) : nullptr;
  return e && *e ? e : nullptr;
}

void Ctx::host_stamp(const char* tag) {
  if (!host_trace_on) return;
  host_stamps.emplace_back(tag, std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count());
}
void Ctx::host_stamps_print() {
  if (!host_trace_on || host_stamps.empty()) return;
  fprintf(stderr, "[host trace]");
  for (size_t i = 0; i < host_stamps.size(); i++)
    fprintf(stderr, " %s +%.1f", host_stamps[i].first, i ? host_stamps[i].second - host_stamps[i - 1].second : 0.0);
  fprintf(stderr, " us\n");
  host_stamps.clear();
}

void Ctx::wait_flag(uint32_t seq) {
  volatile uint32_t* f = flag;
  for (uint64_t spin = 0;; spin++) {
    if (*f == seq) return;
    __builtin_ia32_pause();
    if ((spin & 0xfffff) == 0xfffff) {
      // a failed launch never publishes: ask the runtime instead of spinning forever
      hipError_t e = hipStreamQuery(stream);
      if (e == hipSuccess) {
        if (*f == seq) return;
        throw Error(LH_ERR_DEVICE, "kernel finished without publishing its result");
      }
      if (e != hipErrorNotReady) throw Error(LH_ERR_DEVICE, std::string("stream error: ") + hipGetErrorString(e));
    }
  }
}

Event Ctx::live_event() {
  Event e;
  if (!live_pool.empty()) {
    e = std::move(live_pool.back());
    live_pool.pop_back();
  }
  (void)e.get();
  return e;
}
void Ctx::live_resolve(std::vector<ProfRec>& out) {
  LH_HIP(hipStreamSynchronize(stream));
  if (aux_stream) LH_HIP(hipStreamSynchronize(aux_stream));
  for (size_t i = 0; i < live_recs.size();) {
    size_t j = i;
    ProfRec sum = live_recs[i].rec;
    snprintf(sum.name, sizeof sum.name, "%s/batch", live_recs[i].rec.name);
    sum.bytes = sum.muls = sum.items = 0;
    float span = 0;
    for (; j < live_recs.size() && live_recs[j].batch == live_recs[i].batch; j++) {
      LiveRec& r = live_recs[j];
      float ms = 0, end = 0;
      (void)hipEventElapsedTime(&ms, r.e0.get(), r.e1.get());
      (void)hipEventElapsedTime(&end, live_recs[i].e0.get(), r.e1.get());  // (the batch's first launch starts first: the others wait for an event behind it)
      r.rec.ms = ms;
      span = std::max(span, end);
      sum.bytes += r.rec.bytes, sum.muls += r.rec.muls, sum.items += r.rec.items;
      out.push_back(r.rec);
    }
    sum.ms = span;
    out.push_back(sum);
    i = j;
  }
  for (LiveRec& r : live_recs) live_pool.push_back(std::move(r.e0)), live_pool.push_back(std::move(r.e1));
  live_recs.clear();
}

void Ctx::aux_streams() {
  if (aux_stream) return;
  // (the LOWEST priority the device offers: what runs here fills the wave slots the ctx's stream leaves idle)
  int prio_least = 0, prio_greatest = 0;
  LH_HIP(hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest));
  aux_stream.create(hipStreamNonBlocking, prio_least);
  (void)aux_ev.get();
}
ScFinishArgs Ctx::finish_for_aux(uint32_t grid, uint32_t seq) {
  ScFinishArgs f{ticket.as<uint32_t>() + 16, (uint32_t)(aux_ticket_base + grid - 1), nullptr, flag.as<uint32_t>() + 4, seq, nullptr, 0, nullptr};
  if (grid > 1) aux_ticket_base += grid;
  return f;
}
void Ctx::wait_flag_aux(uint32_t seq) {
  volatile uint32_t* f = flag.as<uint32_t>() + 4;
  for (uint64_t spin = 0;; spin++) {
    if (*f == seq) return;
    __builtin_ia32_pause();
    if ((spin & 0xfffff) == 0xfffff) {
      hipError_t e = hipStreamQuery(aux_stream ? aux_stream : stream);
      if (e == hipSuccess) {
        if (*f == seq) return;
        throw Error(LH_ERR_DEVICE, "kernel on the aux stream finished without publishing its result");
      }
      if (e != hipErrorNotReady) throw Error(LH_ERR_DEVICE, std::string("aux stream error: ") + hipGetErrorString(e));
    }
  }
}

ScFinishArgs Ctx::finish_for(uint32_t grid, Fr* out_host, uint32_t seq, double stored_bytes) {
  // (the lane buffer serves launches of at most 16 sums per workgroup, one at a time: the kernels of this ctx's stream)
  // Every launch hands over in lanes (measured on 2^24 AND lookups: no launch 58.9-59.0 ms, launches that store >= 2^28 bytes
  // 58.0, >= 2^25 bytes 57.4, every launch 57.1; 2^22 range 15.67 / 15.37 / 15.30; 2^20: within the noise).
  // LH_FIN_LANES_MIN_BYTES: the smallest launch (by the bytes its workgroups store) that does - development A/B; -1: none
  const double lanes_min = knob(Knob::FIN_LANES_MIN_BYTES);
  const bool lanes = lanes_min >= 0 && stored_bytes >= lanes_min && grid > 1 && (uint64_t)grid * 16 <= FIN_LANE_SUMS;
  ScFinishArgs f{ticket, (uint32_t)(ticket_base + grid - 1), out_host, flag, seq, nullptr, 0, lanes ? fin_lanes.as<uint64_t>() : nullptr};
  if (sc_redirect) f.out_host = sc_redirect, f.flag = ticket.as<uint32_t>() + 8, f.wide = sc_wide, f.tag = sc_tag;  // sharded round: a device word nobody waits on
  if (grid > 1) ticket_base += grid;  // single-workgroup launches draw no ticket
  return f;
}

// one 16-byte store per chunk (aligned SSE stores are single-copy atomic on every x86-64 with AVX)
static inline void store_chunk(TailChunk* dst, uint32_t a, uint32_t b, uint32_t c_, uint32_t d) {
  _mm_store_si128((__m128i*)dst, _mm_set_epi32((int)d, (int)c_, (int)b, (int)a));
}
static inline void load_chunk(const TailChunk* src, uint32_t w[4]) {
  _mm_store_si128((__m128i*)w, _mm_load_si128((const __m128i*)src));
}

void Ctx::mbox_send(const Fr& r, uint32_t seq) {
  TailMbox* m = mbox();
  store_chunk(&m->c[0], seq, r.l[0], r.l[1], r.l[2]);
  store_chunk(&m->c[1], seq, r.l[3], r.l[4], r.l[5]);
  store_chunk(&m->c[2], seq, r.l[6], r.l[7], 0);
}

void Ctx::mbox_abort() {
  TailMbox* m = mbox();
  for (int j = 0; j < 3; j++) store_chunk(&m->c[j], SC_TAIL_ABORT, 0, 0, 0);
}

void Ctx::gkr_boxes() {
  if (gkr_relay) return;
  gkr_mbox.alloc(GKR_MSG_CHUNKS * sizeof(TailChunk));
  memset(gkr_mbox.get(), 0, GKR_MSG_CHUNKS * sizeof(TailChunk));
  gkr_relay.alloc((4 + GKR_MSG_CHUNKS) * sizeof(TailChunk));
  LH_HIP(hipMemset(gkr_relay, 0, (4 + GKR_MSG_CHUNKS) * sizeof(TailChunk)));
}
void Ctx::gkr_send_layer(const Fr* vals, size_t count, uint32_t seq) {
  LH_REQUIRE(3 * count <= GKR_MSG_CHUNKS, LH_ERR_ARG, "resident layers: layer message too long");
  for (size_t i = 0; i < count; i++) {
    const Fr& r = vals[i];
    TailChunk* box = gkr_mbox.as<TailChunk>() + 3 * i;
    store_chunk(box + 0, seq, r.l[0], r.l[1], r.l[2]);
    store_chunk(box + 1, seq, r.l[3], r.l[4], r.l[5]);
    store_chunk(box + 2, seq, r.l[6], r.l[7], 0);
  }
}
void Ctx::gkr_abort() {
  mbox_abort();
  if (gkr_mbox) store_chunk(gkr_mbox.as<TailChunk>(), SC_TAIL_ABORT, 0, 0, 0);
}
void Ctx::gkr_resync() {
  if (gkr_relay) LH_HIP(hipMemsetAsync(gkr_relay, 0, (4 + GKR_MSG_CHUNKS) * sizeof(TailChunk), stream));
  if (gkr_mbox) memset(gkr_mbox.get(), 0, GKR_MSG_CHUNKS * sizeof(TailChunk));
  k_sc_tail_resync(*this);
}

void Ctx::wait_chunks(const TailChunk* chunks, size_t count, uint32_t seq, Fr* out) {
  (void)wait_chunks_or(chunks, count, seq, seq, out);
}
bool Ctx::wait_chunks_or(const TailChunk* chunks, size_t count, uint32_t seq, uint32_t alt, Fr* out) {
  alignas(16) uint32_t w[4];
  size_t have = 0;  // chunks 0..have-1 carry `seq` and are copied out
  bool gone = false;
  for (uint64_t spin = 0;; spin++) {
    while (have < count) {
      load_chunk(chunks + have, w);
      if (have == 0 && alt != seq && w[0] == alt) return false;
      if (w[0] != seq) break;
      Fr& f = out[have / 3];
      const size_t j = have % 3;
      f.l[3 * j] = w[1], f.l[3 * j + 1] = w[2];
      if (j < 2) f.l[3 * j + 2] = w[3];
      have++;
    }
    if (have == count) return true;
    __builtin_ia32_pause();
    if ((spin & 0xfffff) == 0xfffff) {
      hipError_t e = hipStreamQuery(stream);
      if (e == hipSuccess) {
        if (gone) throw Error(LH_ERR_DEVICE, "kernel finished without publishing its result");
        gone = true;  // one more look at the chunks: they may have landed between the last look and the query
        spin = 0xffffe;
        continue;
      }
      if (e != hipErrorNotReady) throw Error(LH_ERR_DEVICE, std::string("stream error: ") + hipGetErrorString(e));
    }
  }
}

void Ctx::d2h(void* dst, const void* d_src, size_t bytes) {
  if (!bytes) return;
  if (bytes > ((size_t)8 << 20)) {  // bulk: let the runtime stream it
    LH_HIP(hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, stream));
    sync();
    return;
  }
  void* via = stage.reserve(bytes, (size_t)1 << 20);
  LH_HIP(hipMemcpyAsync(via, d_src, bytes, hipMemcpyDeviceToHost, stream));
  sync();
  memcpy(dst, via, bytes);
}

// ------------------------------------------------------------------ HostWorker
struct HostWorker::Impl {
  std::mutex mu;
  std::condition_variable cv, idle_cv;
  std::vector<std::function<void()>> queue;
  size_t head = 0;
  bool busy = false, stop = false;
  std::thread th;
  void loop() {
    for (;;) {
      std::function<void()> fn;
      {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return stop || head < queue.size(); });
        if (head >= queue.size()) return;  // (stop, and nothing left)
        fn = std::move(queue[head++]);
        if (head == queue.size()) queue.clear(), head = 0;
        busy = true;
      }
      try {
        fn();
      } catch (...) {  // (tasks report their own errors; nothing may escape a thread)
      }
      {
        std::lock_guard<std::mutex> lk(mu);
        busy = false;
      }
      idle_cv.notify_all();
    }
  }
};
HostWorker::HostWorker() : impl_(new Impl()) { impl_->th = std::thread([this] { impl_->loop(); }); }
HostWorker::~HostWorker() {
  {
    std::lock_guard<std::mutex> lk(impl_->mu);
    impl_->stop = true;
  }
  impl_->cv.notify_all();
  if (impl_->th.joinable()) impl_->th.join();
  delete impl_;
}
void HostWorker::submit(std::function<void()> fn) {
  {
    std::lock_guard<std::mutex> lk(impl_->mu);
    impl_->queue.push_back(std::move(fn));
  }
  impl_->cv.notify_one();
}
void HostWorker::wait() {
  std::unique_lock<std::mutex> lk(impl_->mu);
  impl_->idle_cv.wait(lk, [&] { return !impl_->busy && impl_->head >= impl_->queue.size(); });
}

void Ctx::phase_times_resolve() {
  if (!phase_ev_pending) return;
  phase_ev_pending = false;
  // ev[0] = start of the prove, ev[k + 1] = end of phase k (k = 0..6); [7] stays 0, [8] (total) is the host's wall clock
  if (!phase_ev[0].created()) return;
  LH_HIP(hipEventSynchronize(phase_ev[7].get()));
  for (int k = 0; k < 7; k++) {
    float ms = 0;
    LH_HIP(hipEventElapsedTime(&ms, phase_ev[k].get(), phase_ev[k + 1].get()));
    lasso_ms[k] = (double)ms;
  }
}

// ------------------------------------------------------------------ host worker pool
// Every parallel_for publishes ONE immutable job object (function, item count, its own claim and completion
// counters).  A worker copies the shared_ptr under the mutex and claims indices only from that job's counter, so a
// worker that wakes late works on its own (already finished) job and can never draw an index of the next generation.
namespace {
struct HostJob {
  std::function<void(size_t)> fn;
  size_t n = 0;
  std::atomic<size_t> next{0}, done{0};
  void run() {
    size_t i;
    while ((i = next.fetch_add(1, std::memory_order_relaxed)) < n) {
      fn(i);
      done.fetch_add(1, std::memory_order_release);
    }
  }
};
struct HostPool {
  std::mutex mu;
  std::condition_variable cv;
  std::atomic<uint64_t> gen{0};
  uint64_t spin_gen = 0;       // bumped by prewake(): `spin_want` sleeping workers wake up and poll `gen` until `spin_until`
  int spin_want = 0;
  std::chrono::steady_clock::time_point spin_until;
  std::atomic<int> spinning{0};
  std::shared_ptr<HostJob> job;
  unsigned workers = 0;
  // the CPUs this process may run on (taskset, a cgroup, Context.bind_host: fewer than the machine's)
  static unsigned usable_cpus() {
    cpu_set_t set;
    CPU_ZERO(&set);
    if (sched_getaffinity(0, sizeof(set), &set) == 0 && CPU_COUNT(&set) > 0) return (unsigned)CPU_COUNT(&set);
    const unsigned hw = std::thread::hardware_concurrency();
    return hw ? hw : 1;
  }
  HostPool() {
    unsigned hw = usable_cpus();
    // (an MSM batch hands ~25-40 window combines of ~70 us each to this pool at the end of a commit or an opening - the
    // GPU idles meanwhile: one round of them, not three, where the host has the cores; LH_HOST_THREADS overrides)
    const unsigned cap = (unsigned)std::max(0, (int)knob(Knob::HOST_THREADS) - 1);
    workers = hw > 1 ? std::min(cap, hw - 1) : 0;
    for (unsigned i = 0; i < workers; i++) std::thread([this] { worker(); }).detach();
  }
  void worker() {
    uint64_t seen = 0, seen_spin = 0;
    bool was_spinning = false;
    for (;;) {
      std::shared_ptr<HostJob> mine;
      bool spin = false;
      std::chrono::steady_clock::time_point until;
      {
        std::unique_lock<std::mutex> lk(mu);
        // (`spinning` only changes under the lock: a poster that counts the pollers under the lock counts exactly the
        // workers that will look at `gen` again before they sleep)
        if (was_spinning) spinning--, was_spinning = false;
        cv.wait(lk, [&] { return gen.load(std::memory_order_relaxed) != seen || (spin_gen != seen_spin && spin_want > 0); });
        if (gen.load(std::memory_order_relaxed) != seen) {
          seen = gen.load(std::memory_order_relaxed);
          seen_spin = spin_gen;
          mine = job;
        } else {  // woken ahead of a job that is about to come: poll for it instead of sleeping through its arrival
          seen_spin = spin_gen;
          spin_want--;
          spin = true;
          until = spin_until;
          spinning++, was_spinning = true;
        }
      }
      if (spin) {
        while (gen.load(std::memory_order_acquire) == seen && std::chrono::steady_clock::now() < until) __builtin_ia32_pause();
        continue;  // (takes the job under the lock if one came, sleeps again otherwise)
      }
      if (mine) mine->run();
    }
  }
  // a parallel_for of about `count` items will be posted within `us` microseconds: have workers awake and polling by then
  // (waking a sleeping thread costs the poster ~50 us of the ~70 us an item takes)
  void prewake(size_t count, unsigned us) {
    if (!workers || count <= 1) return;
    // (polling threads burn a core each: at most an eighth of the host's - eight ranks may share it, one process per GPU)
    static const size_t spin_cap = std::max<size_t>(1, usable_cpus() / 8);
    int want;
    {
      std::lock_guard<std::mutex> lk(mu);
      want = (int)std::min<size_t>(std::min<size_t>(count - 1, workers), spin_cap) - spinning;
      if (want <= 0) return;
      spin_gen++;
      spin_want = want;
      spin_until = std::chrono::steady_clock::now() + std::chrono::microseconds(us);
    }
    if (want >= (int)workers) cv.notify_all();
    else
      for (int i = 0; i < want; i++) cv.notify_one();
  }
  void parallel_for(size_t count, const std::function<void(size_t)>& f) {
    auto j = std::make_shared<HostJob>();
    j->fn = f;  // a copy: the job outlives the caller's frame for workers that wake late
    j->n = count;
    bool enough_awake;
    {
      std::lock_guard<std::mutex> lk(mu);
      enough_awake = (size_t)spinning + 1 >= count;  // (decided under the lock: see worker())
      job = j;
      gen.fetch_add(1, std::memory_order_release);
      spin_want = 0;
    }
    if (!enough_awake) cv.notify_all();  // (polling workers see `gen` move by themselves)
    j->run();
    while (j->done.load(std::memory_order_acquire) != count) __builtin_ia32_pause();
    {
      std::lock_guard<std::mutex> lk(mu);
      if (job == j) job.reset();
    }
  }
};
}  // namespace

static HostPool& host_pool() {
  static HostPool* pool = new HostPool();  // never destroyed: workers sleep on the condition variable
  return *pool;
}
void host_parallel_for(size_t n, const std::function<void(size_t)>& fn) {
  if (n <= 1) {
    for (size_t i = 0; i < n; i++) fn(i);
    return;
  }
  host_pool().parallel_for(n, fn);
}
void host_parallel_prewake(size_t n, unsigned us) { host_pool().prewake(n, us); }

}  // namespace lh
