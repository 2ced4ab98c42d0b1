// Host half of the prover: mirrors the reference's trait surface for the hot path
// (piop::sum_check, piop::gkr, pcs::multilinear::kzg) on top of the device kernels.
#pragma once
#include <string.h>
#include <algorithm>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <vector>
#include "dev.hpp"
#include "ff_host.hpp"

namespace lh {

const char* get_last_error();

typedef host::Fr HFr;
typedef host::G1Affine HG1;

static inline Fr dev(const HFr& f) {
  Fr r;
  memcpy(&r, &f, 32);
  return r;
}
static inline HFr hst(const Fr& f) {
  HFr r;
  memcpy(&r, &f, 32);
  return r;
}

// ------------------------------------------------------------------ hash + transcript
struct Keccak256 {
  static constexpr int RATE = 136;
  uint64_t state[25] = {0};
  uint8_t buf[RATE];
  size_t buf_len = 0;
  void absorb_block(const uint8_t* block);
  void update(const uint8_t* data, size_t len);
  void finalize_reset(uint8_t out[32]);
};

struct KeccakTranscript {
  lh_transcript vt;  // must stay the first member: lh_transcript* <-> KeccakTranscript*
  Keccak256 hash;
  std::vector<uint8_t> stream;
  size_t pos = 0;  // read cursor (from_proof transcripts)
  KeccakTranscript();
};

// typed view over the callback table (util/transcript.rs:15-97)
struct Transcript {
  lh_transcript* t;
  explicit Transcript(lh_transcript* t_) : t(t_) {
    LH_REQUIRE(t && t->write_field_element && t->common_field_element && t->squeeze_challenge &&
                   t->write_commitment && t->common_commitment,
               LH_ERR_ARG, "transcript callback table is incomplete");
  }
  void check(int rc) {
    if (rc != LH_OK) throw Error(rc, get_last_error()[0] ? get_last_error() : "transcript callback failed");
  }
  void write_field_element(const HFr& f) { check(t->write_field_element(t->user, (const lh_fr*)&f)); }
  void write_field_elements(const std::vector<HFr>& fs) {
    for (auto& f : fs) write_field_element(f);
  }
  void common_field_element(const HFr& f) { check(t->common_field_element(t->user, (const lh_fr*)&f)); }
  HFr squeeze_challenge() {
    HFr f;
    check(t->squeeze_challenge(t->user, (lh_fr*)&f));
    return f;
  }
  std::vector<HFr> squeeze_challenges(size_t n) {
    std::vector<HFr> v(n);
    for (auto& f : v) f = squeeze_challenge();
    return v;
  }
  void write_commitment(const HG1& p) { check(t->write_commitment(t->user, (const lh_g1*)&p)); }
  void write_commitments(const std::vector<HG1>& ps) {
    for (auto& p : ps) write_commitment(p);
  }
  void common_commitment(const HG1& p) { check(t->common_commitment(t->user, (const lh_g1*)&p)); }
  // TranscriptRead (util/transcript.rs:45-97)
  HFr read_field_element() {
    LH_REQUIRE(t->read_field_element, LH_ERR_ARG, "transcript cannot read (write-only callback table)");
    HFr f;
    check(t->read_field_element(t->user, (lh_fr*)&f));
    return f;
  }
  std::vector<HFr> read_field_elements(size_t n) {
    std::vector<HFr> v(n);
    for (auto& f : v) f = read_field_element();
    return v;
  }
  HG1 read_commitment() {
    LH_REQUIRE(t->read_commitment, LH_ERR_ARG, "transcript cannot read (write-only callback table)");
    HG1 p;
    check(t->read_commitment(t->user, (lh_g1*)&p));
    return p;
  }
  std::vector<HG1> read_commitments(size_t n) {
    std::vector<HG1> v(n);
    for (auto& p : v) p = read_commitment();
    return v;
  }
};

// PolynomialCommitmentScheme::batch_verify of the PCS a backend is generic over
typedef std::function<void(size_t num_vars, const HG1* comms, size_t num_comms, const HFr* points, size_t num_points,
                           const lh_evaluation* evals, size_t num_evals, Transcript& tr)>
    PcsBatchVerify;
// optional, for a PCS whose commitments are not G1 points (Brakedown: 32-byte Merkle roots that cross the transcript
// unabsorbed): reads n commitments, each into the first bytes of a 64-byte HG1 slot that only its own batch_verify interprets
typedef std::function<std::vector<HG1>(Transcript& tr, size_t n)> PcsReadCommitments;
// what the verifiers (Lasso, HyperPlonk) need from their PCS: the verifier-side twin of Pcs below.  Every scheme builds its
// own next to its batch_verify (mkzg_verifier, zeromorph_verifier, gemini_verifier, ipa_verifier, hyrax_verifier); the param
// it is built from must outlive it
struct PcsVerifier {
  PcsBatchVerify batch_verify;
  // points per commitment (Hyrax's rows): every commitment is read as that many points, a HyperPlonk verifier param holds
  // that many per poly (poly-major), and batch_verify gets the commitments as vectors, commitment-major
  size_t chunks = 1;
  PcsReadCommitments read_commitments;  // optional (default: Transcript::read_commitments)
};

// ------------------------------------------------------------------ poly helpers (host side, tiny inputs)
std::vector<HFr> host_eq_xy(const std::vector<HFr>& y);           // multilinear.rs:91-127
HFr host_eq_xy_eval(const HFr* x, const HFr* y, size_t n);         // sum_check.rs:112-121
// evaluations of `count` device tables at `point` (multilinear.rs:137-156)
std::vector<HFr> evaluate_polys(Ctx&, const Fr* const* d_polys, size_t count, size_t num_vars, const HFr* point);

// ------------------------------------------------------------------ piop::sum_check
struct SumCheckResult {
  std::vector<HFr> challenges;  // x
  std::vector<HFr> evals;       // every poly at x (classic.rs:143-149)
  bool u32_terms_built = false;  // given ScOptions::u32_terms: the tables of d_polys hold the polys in full
};
// `sum_is_exact`: the caller computed `sum` from these very tables (the provers' internal sum-checks: Surge, the GKR
// layers): eq factoring then trusts it from round 0 on; a claim from outside (the C-ABI) is checked first (EqFactoring)
// `rw` (optional): the expression is a grand-product layer over (A_i, A_i + 1) tree pairs written over the A tables
// alone (dev.hpp ScRwRound; polys = l_0, r_0, l_1, r_1, ...): its streaming rounds run the dedicated kernel
struct ScRwPairs {
  uint32_t num_pairs;
  HFr cs[SC_RW_MAX_PAIRS], k[SC_RW_MAX_PAIRS];
  HFr const_total;  // sum of the constants the factorisation leaves behind: added to q at every point
};
// `u32` (optional): the single table d_polys[0] has NOT been written - its values are this 32-bit column.  The sum-check
// either runs its first three rounds from the column (sumcheck.cpp: the sums of k_inner_products_small_quads are rounds 0
// and 1, k_sc_round_u32_bind2 is round 2) or fills the table itself.
struct ScU32 {
  const uint32_t* col = nullptr;
  bool have_sums = false;
  Fr odd, s2, s3;  // (when have_sums: out_host[1..3] of k_inner_products_small_quads against the sum-check's E_0)
};
// `u32_terms` (optional), for the batch-opening shape sum_m eq(y_m, .) poly_m: poly b = sum_k w[k] col[k] over 32-bit
// columns (entries beyond len[k] are zero) and d_polys[b] has NOT been written.  The sum-check runs its first three rounds
// from the columns (sumcheck.cpp: k_inner_products_quads, k_lincomb_bind2) or fills the tables itself (k_lincomb_mixed)
// and says so in SumCheckResult::u32_terms_built.
struct ScU32Terms {
  struct Poly {
    std::vector<const uint32_t*> col;
    std::vector<size_t> len;
    std::vector<Fr> w;
  };
  std::vector<Poly> polys;
};
// `sharded` (inside a sharded proof, dev.hpp Shard): d_polys are this rank's shards of num_vars-variable tables; same
// messages, same result on every rank
struct ScOptions {
  bool sum_is_exact = false;
  bool sharded = false;
  const ScRwPairs* rw = nullptr;
  const ScU32* u32 = nullptr;
  const ScU32Terms* u32_terms = nullptr;
};
SumCheckResult sum_check_prove(Ctx&, int prover_kind, size_t num_vars, const lh_sop& expr, const Fr* const* d_polys,
                               size_t num_polys, const HFr* ys, size_t num_ys, const HFr& sum, Transcript& tr,
                               const ScOptions& opt = ScOptions());

// eq table of y[1..num_vars) (2^(num_vars-1) entries), shared through Ctx::eq_half_cache within one proof; `sharded`: this
// rank's shard of it with the rank's factor of the shard coordinates multiplied in
const Fr* eq_half_lookup(Ctx&, const HFr* y, size_t num_vars, bool sharded = false);
const Fr* eq_half_get(Ctx&, const HFr* y, size_t num_vars, bool sharded = false);  // built (in the arena, at the caller's depth) when absent
struct EqHalfScope {  // forgets, on exit, what was cached after its creation (eq tables and quad sums alike)
  Ctx& c;
  size_t mark, mark_sums;
  explicit EqHalfScope(Ctx& c_) : c(c_), mark(c_.eq_half_cache.size()), mark_sums(c_.quad_sums.size()) {}
  ~EqHalfScope() {
    c.eq_half_cache.resize(mark);
    c.quad_sums.resize(mark_sums);
  }
};
// Will a batch opening of num_vars-variable polys given as 32-bit columns take its rounds 0 and 1 from the columns' quad sums
// (sumcheck.cpp, ScOptions::u32_terms)?  What can be known without the opening's expression: the sum-check adds its own
// conditions on the round kernels; the argument asks before it decides how to make its evaluations.
bool sc_open_column_rounds(const Ctx&, size_t num_vars, bool sharded);
// The proof's table of quad sums (Ctx::quad_sums): S_0..S_3 of the column (col, len) at the point y, or null
const Fr* quad_sums_lookup(const Ctx&, const uint32_t* col, size_t len, const HFr* y, size_t num_vars);
void quad_sums_put(Ctx&, const uint32_t* col, size_t len, const HFr* y, size_t num_vars, const HFr s[4]);
// evals[k] = cols[k](y) for `count` columns of 2^num_vars entries, num_vars >= 3, from ONE pass that makes every column's
// quad sums against eq_half = the eq table of y[1..] (k_quad_sums) and leaves them in the table:
//   col(y) = (1-y0)(1-y1) S_0 + y0 (1-y1) S_1 + (1-y0) y1 S_2 + y0 y1 S_3
void quad_sums_evaluate(Ctx&, const uint32_t* const* cols, size_t count, const HFr* y, size_t num_vars, const Fr* eq_half, HFr* evals);

// the round loop shared by every sum-check front end (sumcheck.cpp)
typedef std::function<void(const Fr* const*, Fr* const*, const Fr&, bool, size_t, Fr*)> RoundFn;
// Eq factoring of the streaming rounds.  eq(y, x) = prod_i eq(y_i, x_i), so in round j (prefix bound to rho):
//   eq(y, (rho, X, b)) = S_j * eq(y_j, X) * E_j[b],   S_j = prod_{i<j} eq(y_i, rho_i),   E_j = eq table over variables > j.
// The round polynomial of  eq * g  is therefore  p(X) = S_j eq(y_j, X) q(X)  with  q(X) = sum_b E_j[b] g(rho, X, b)  of one
// degree less: the device evaluates q at one point fewer, reads ONE eq entry per pair instead of streaming and binding a
// whole eq table, and the host rebuilds exactly the reference's message p(0..D) (field arithmetic is exact: same bytes).
// q(0) follows from the claim:  claim / S_j = (1 - y_j) q(0) + y_j q(1).  When the rounds leave the streaming kernel the eq
// table is materialised once in its "previous round" form  S_{j-1} * E_{j-2}  and the standard path continues.
struct EqFactoring {
  struct One {
    size_t table;                    // index of the eq table in `cur` (filled at the switch)
    const HFr* y;                    // the eq point (num_vars coordinates)
    std::vector<const Fr*> level;    // level[j] = E_j, 2^(num_vars - 1 - j) entries on the device
    HFr S, S_prev;                   // S_j, S_{j-1}
    std::vector<HFr> q;              // q(0..) of the current round
  };
  std::vector<One> eqs;    // global-eq shape: one entry; per-term shape (sum_m eq_m * poly_m): one per term, in term order
  bool per_term = false;
  bool trusted_claim = false;  // the claim is known to be the true sum: no check (and no extra point) in round 0
  // set by the round loop when round 0 found the claim NOT to be the true sum (the reference still sends the true p(1..D),
  // eval.rs:129 - benches/zero_check.rs proves a false claim over random tables): every round then evaluates q at D points
  // and takes nothing from the claim; the eq table stays factored
  bool untrusted = false;
  std::vector<HFr> inv_1my;  // global-eq shape: (1 - y_j)^-1 for every round
  HFr c;                     // global-eq shape: claim / S_j
  HFr add_const;             // set by `round`: a constant the kernel left out of every q value (ScRwPairs::const_total)
  // global-eq shape beside a LINEAR part (the zero-check of HyperPlonk, expr.cpp): the round polynomial is
  //   p(X) = A(X) + kappa S_j eq(y_j, X) q(X),  A(X) = lin0 + X (lin1 - lin0)
  // with lin0 / lin1 = the linear part's sums over the even / odd entries of this round's tables, set by `round`;
  // `c` then is the eq part's claim alone (round 0: set by `round` too, (sum - lin0 - lin1) / kappa)
  HFr kappa = HFr::one(), lin0 = HFr::zero(), lin1 = HFr::zero();
  // would this round run the streaming kernel (else the eq tables are materialised and the standard path takes over)
  std::function<bool(bool bind, size_t size)> streams;
  // launches the factored round; device output: q(1..points) (global-eq shape; points = D - 1, or D in round 0 where the
  // claim is checked rather than trusted) or q_m(0), q_m(1) per term
  std::function<void(const Fr* const* in, Fr* const* out, const Fr& r, bool bind, size_t size, size_t round, int points,
                     Fr* out_host)>
      round;
  // the rest of the sum-check inside the resident kernel (kernels_gkr.hip, GKR_F_* tail mode) when the shape allows it:
  // `cur` the current tables (pending their bind with r_prev when `bind`), n0 entries each after that bind, `round` the
  // first resident round, `claim` the running claim.  Appends the challenges and fills the evaluations; false: not taken.
  std::function<bool(const std::vector<const Fr*>& cur, bool bind, const HFr& r_prev, size_t n0, size_t round, const HFr& claim,
                     Transcript& tr, SumCheckResult& res)>
      resident_tail;
};
SumCheckResult sum_check_loop(Ctx&, int prover_kind, size_t num_vars, int degree, std::vector<const Fr*> cur,
                              const std::vector<char>& used, size_t num_polys, const HFr& sum, Transcript& tr,
                              bool sharded, const RoundFn& round_fn, const ScRound* tail_rd = nullptr,
                              EqFactoring* ef = nullptr);
// general Expression (util/expression.rs) through EvaluationsProver; evals = every poly at x
SumCheckResult sum_check_prove_expr(Ctx&, size_t num_vars, const lh_expr& expr, const Fr* const* d_polys,
                                    size_t num_polys, const HFr* challenges, size_t num_challenges, const HFr* ys,
                                    size_t num_ys, const HFr& sum, Transcript& tr, bool sharded = false);

// one proof over several GPUs (dev.hpp Shard): tables are this rank's shards, results are global
std::vector<HFr> evaluate_polys(Ctx&, const Fr* const* d_polys, size_t count, size_t num_vars, const HFr* point, bool sharded);
void comm_sum_fr(Ctx&, HFr* v, size_t n);
void comm_sum_points(Ctx&, HG1* pts, size_t n);
void comm_gather_tables(Ctx&, const Fr* local_block, size_t count, size_t n_local, size_t block, Fr* const* out);
void comm_gather_concat(Ctx&, const Fr* local, size_t n_local, Fr* out);
// this rank's shard of eq_xy(y[first..num_vars)) (the shard coordinates dropped, the rank's factor multiplied in)
void eq_xy_shard(Ctx&, const Shard&, const HFr* y, size_t num_vars, size_t first, Fr* out_local);

// ------------------------------------------------------------------ piop::gkr
struct FracSumCheckResult {
  std::vector<HFr> p_xs, q_xs, x;
};
// d_p_up / d_q_up (optional, both or neither): per fraction the level above the leaves (2^(num_vars-1) nodes, Layer::up of the
// leaves) when the caller made it together with the leaves; ignored for num_vars == 1, which has no such level
FracSumCheckResult prove_fractional_sum_check(Ctx&, size_t num_batching, size_t num_vars,
                                              const HFr* const* claimed_p_0s, const HFr* const* claimed_q_0s,
                                              const Fr* const* d_ps, const Fr* const* d_qs, Transcript& tr,
                                              const Fr* const* d_p_up = nullptr, const Fr* const* d_q_up = nullptr);
struct GrandProductResult {
  std::vector<HFr> roots, claims;
  std::vector<std::vector<HFr>> points;
};
// d_level_up (optional): per tree the level above the leaves (2^(num_vars-1) nodes, node i = leaf[i] * leaf[i + half]) when
// the caller made it together with the leaves, else null
// plus_one (optional): plus_one[b] != 0 says that tree b's leaves are tree (b - 1)'s leaves + 1, entry by entry (same
// depth; Lasso's write set over its read set).  The leaf layer of such a pair then runs over tree (b - 1)'s tables
// alone (dev.hpp ScRwRound) and d_leaves[b] is never read (it may be null; d_level_up[b] must be given).
// `trees_built` (optional) is called once, when the trees are built and the layer sum-checks start: the latency-bound
// stretch of a Lasso prove, where lasso_prove starts the opening's precommit
GrandProductResult prove_grand_product(Ctx&, size_t num_trees, const Fr* const* d_leaves, const size_t* num_vars,
                                       Transcript& tr, const Fr* const* d_level_up = nullptr,
                                       const uint8_t* plus_one = nullptr,
                                       const std::function<void()>& trees_built = nullptr);
// from this many variables on a caller makes the level above a tree's leaves together with them (the tree builder takes the
// level from 11 variables on)
constexpr size_t GP_LEVEL_UP_MIN_VARS = 12;

// ------------------------------------------------------------------ pcs::multilinear::kzg
struct Srs {
  DevMem d_eqs;  // flat: level k at offset 2^k - 1
  size_t num_vars = 0;
  const G1Affine* eq(size_t k) const { return d_eqs.as<G1Affine>() + (((size_t)1 << k) - 1); }
  // this rank's share of the bases of every sharded level (sharded proving; built on first use)
  mutable std::vector<DevMem> shard_levels;
  mutable int shard_rank = -1;
  mutable size_t shard_R = 0, shard_j = 0;
  // sum of all bases of a level (mkzg_open over small-valued columns), computed on first use
  mutable std::map<size_t, HG1> level_sums;  // (guarded by one process-wide mutex, open_columns.hpp srs_cache_mu)
  mutable std::map<size_t, HG1> shard_level_sums;  // the same over this rank's share of a sharded level
  // window tables of whole levels (dev.hpp MsmJob::win_table; Options::msm_window_tables), built on first use
  struct WinTable {
    DevMem d;  // (empty: the level has no table)
    uint32_t c = 0, W = 0;
  };
  mutable std::map<size_t, WinTable> win_tables;
};
// the window table of a level (nullptr: tables are off for this level - Options::msm_window_tables - or do not fit)
const Srs::WinTable* srs_window_table(Ctx&, const Srs&, size_t level);
const G1Affine* srs_shard_level(Ctx&, const Srs&, size_t level);  // this rank's share of a level's bases (sharded proofs)
Srs mkzg_setup(Ctx&, const HFr* ss, size_t num_vars);
std::vector<HG1> mkzg_batch_commit(Ctx&, const Srs&, const Fr* const* d_polys, size_t num_polys, size_t num_vars);
std::vector<HG1> mkzg_batch_commit_u32(Ctx&, const Srs&, const uint32_t* const* d_polys, size_t num_polys,
                                       size_t num_vars);
struct SmallOpen;
// small (optional): d_poly = sum_k coef[k] * cols[k] with small-valued columns: the largest quotient is then committed
// column by column from 32-bit differences (mkzg.cpp, open_columns.cpp)
HFr mkzg_open(Ctx&, const Srs&, const Fr* d_poly, size_t num_vars, const HFr* point, Transcript& tr,
              const SmallOpen* small = nullptr);
// a poly handed over as its small-valued u32 column (`len` entries, zero beyond): Lasso's dim / read_ts / E / final_cts
// reach the batch opening without a field-element view (d_polys[i] may then be null)
struct SmallLinear {  // column = sum_k coeff[k] * (the column of poly[k]) entry by entry (poly: indices of the same opening)
  std::vector<size_t> poly;
  std::vector<HFr> coeff;
};
struct SmallPoly {
  const uint32_t* ptr = nullptr;
  size_t len = 0;
  uint32_t bits = 0;  // every entry < 2^bits when the caller knows (0: unknown)
  // optional: this column is an exact linear combination of other columns of the opening (Lasso's output a = g(E) under a
  // linear g): the small-column opening then folds its coefficient into theirs and never touches it
  const SmallLinear* linear = nullptr;
};
void mkzg_batch_open(Ctx&, const Srs&, size_t num_vars, const Fr* const* d_polys, size_t num_polys,
                     const HFr* points, size_t num_points, const lh_evaluation* evals, size_t num_evals,
                     Transcript& tr, const SmallPoly* small = nullptr);

// g' of a batch opening whose polys are ALL small-valued columns: g' = sum_k coef[k] * cols[k] (scalar coefficients)
struct SmallOpen {
  std::vector<SmallPoly> cols;
  std::vector<HFr> coef;
  // the same g' as a combination of field-element tables (the merged polys of the batch opening): when the opening is
  // handed a null g', it forms what it needs from these (the first fold directly, g' itself only on the plain route)
  std::vector<const Fr*> merged;
  std::vector<Fr> merged_w;
  // the merged tables may not have been written yet (the batch opening's sum-check ran from the columns: sumcheck.cpp,
  // ScOptions::u32_terms): whoever needs them calls this first (null: they are there)
  std::function<void()> ensure_merged;
};
// Options::open_precommit: commit the challenge-free half of the coming batch opening's column route on the ctx's helper
// ctx, starting now (the opening's polys, their small columns and the (poly, point) pairs as mkzg_batch_open will get them;
// the evaluations' values are not used).  mkzg_open picks the results up when they fit, and commits as before when not.
// `staged` >= 0 (Options::open_precommit_stages; the caller is behind the last accumulation launch of its commit batch -
// msm_batch's acc_queued -, 1: a half of it on the aux stream): the helper's differences, digits and sort start once those
// launches have left the chip, its accumulation only from open_precommit_release on (or when the opening takes the plan).
// Returns whether a staged precommit is under way.
bool open_precommit_start(Ctx&, const Srs&, size_t num_vars, const SmallPoly* small, size_t num_polys,
                          const lh_evaluation* evals, size_t num_evals, int staged = -1);
// `open_small` (optional) is called instead of `open` when every opened poly came as a small-valued column
void additive_batch_open(Ctx&, size_t num_vars, const Fr* const* d_polys, size_t num_polys, const HFr* points,
                         size_t num_points, const lh_evaluation* evals, size_t num_evals, Transcript& tr,
                         const std::function<void(const Fr* g_prime, const HFr* point)>& open,
                         const SmallPoly* small = nullptr,
                         const std::function<void(const Fr* g_prime, const HFr* point, const SmallOpen&)>& open_small = nullptr);

// ------------------------------------------------------------------ pcs::multilinear::zeromorph over pcs::univariate::kzg
struct USrs {  // UnivariateKzgParam (univariate/kzg.rs:38-66): powers_of_s_g1 on the device
  DevMem d_powers;
  size_t size = 0;
};
USrs ukzg_setup(Ctx&, const HFr& s, size_t poly_size);
// poly_size: the trim size (zeromorph.rs:90-108): commits use powers[..poly_size], the final quotient powers[size - poly_size..]
std::vector<HG1> zeromorph_batch_commit(Ctx&, const USrs&, size_t poly_size, const Fr* const* d_polys, size_t num_polys,
                                        size_t num_vars);
void zeromorph_open(Ctx&, const USrs&, size_t poly_size, const Fr* d_poly, size_t num_vars, const HFr* point,
                    Transcript& tr);
void zeromorph_batch_open(Ctx&, const USrs&, size_t poly_size, size_t num_vars, const Fr* const* d_polys,
                          size_t num_polys, const HFr* points, size_t num_points, const lh_evaluation* evals,
                          size_t num_evals, Transcript& tr, const SmallPoly* small = nullptr);
// zeromorph.rs:258-296 -> (eval_scalar, q_scalars)
std::pair<HFr, std::vector<HFr>> zeromorph_scalars(const HFr& y, const HFr& x, const HFr& z, const HFr* u, size_t n);
struct ZmVerifierParams;  // ZeromorphKzgVerifierParam (zeromorph.rs:42-65)
ZmVerifierParams* zeromorph_vp_setup(const HFr& s, size_t param_size, size_t poly_size);
ZmVerifierParams* zeromorph_vp_new(const lh_g1& g1, const lh_g2& g2, const lh_g2& s_g2, const lh_g2& s_offset_g2);
void zeromorph_vp_export(const ZmVerifierParams&, lh_g1* g1, lh_g2* g2, lh_g2* s_g2, lh_g2* s_offset_g2);
void zeromorph_vp_free(ZmVerifierParams*);
void zeromorph_verify(const ZmVerifierParams&, const HG1& comm, const HFr* point, size_t num_vars, const HFr& eval,
                      Transcript& tr);
void zeromorph_batch_verify(const ZmVerifierParams&, size_t num_vars, const HG1* comms, size_t num_comms,
                            const HFr* points, size_t num_points, const lh_evaluation* evals, size_t num_evals,
                            Transcript& tr);
PcsVerifier zeromorph_verifier(const ZmVerifierParams&);

// ------------------------------------------------------------------ pcs::univariate::kzg on its own, pcs::multilinear::gemini over it
// (gemini.cpp; verifiers in verifier.cpp).  `poly_size` is the trim size (univariate/kzg.rs:220-240): pp = powers[..poly_size].
// A univariate poly is a coefficient vector of FIXED length on the device: the reference drops leading zero coefficients,
// which changes no commitment (a zero scalar contributes the identity), and checks degrees after dropping them; here the
// length itself must fit the param.
struct UPoly {
  const Fr* d;
  size_t len;
};
std::vector<HG1> ukzg_batch_commit(Ctx&, const USrs&, size_t poly_size, const UPoly* polys, size_t num_polys);
void ukzg_open(Ctx&, const USrs&, size_t poly_size, const UPoly& poly, const HFr& point, Transcript& tr);
void ukzg_batch_open(Ctx&, const USrs&, size_t poly_size, const UPoly* polys, size_t num_polys, const HFr* points,
                     size_t num_points, const lh_evaluation* evals, size_t num_evals, Transcript& tr);
// univariate/kzg.rs:422-555, shared by prover and verifier (host only)
struct UkzgEvalSet {
  std::vector<size_t> polys, points, diffs;
  std::vector<std::vector<HFr>> evals;  // per poly, in the order of `points`
};
struct UkzgEvalSets {
  std::vector<UkzgEvalSet> sets;
  std::vector<size_t> superset;  // ascending
};
UkzgEvalSets ukzg_eval_sets(const lh_evaluation* evals, size_t num_evals);
HFr ukzg_vanishing_eval(const std::vector<size_t>& idx, const HFr* points, const HFr& z);
// -> (normalized set scalars, normalizer)
std::pair<std::vector<HFr>, HFr> ukzg_set_scalars(const std::vector<UkzgEvalSet>& sets, const std::vector<HFr>& powers_of_gamma,
                                                  const HFr* points, const HFr& z);
std::vector<HG1> gemini_batch_commit(Ctx&, const USrs&, size_t poly_size, const Fr* const* d_polys, size_t num_polys,
                                     size_t num_vars);
void gemini_open(Ctx&, const USrs&, size_t poly_size, const Fr* d_poly, size_t num_vars, const HFr* point, Transcript& tr);
void gemini_batch_open(Ctx&, const USrs&, size_t poly_size, size_t num_vars, const Fr* const* d_polys, size_t num_polys,
                       const HFr* points, size_t num_points, const lh_evaluation* evals, size_t num_evals, Transcript& tr,
                       const SmallPoly* small = nullptr);
// development / tests: the folds fs[1..] of a Gemini opening in their arena layout (2^num_vars - 2 coefficients)
void gemini_folds(Ctx&, const Fr* d_poly, size_t num_vars, const HFr* point, Fr* d_out);
struct UkzgVerifierParams;  // UnivariateKzgVerifierParam (univariate/kzg.rs:90-120): g1, g2, [s]_2
UkzgVerifierParams* ukzg_vp_setup(const HFr& s);
UkzgVerifierParams* ukzg_vp_new(const lh_g1& g1, const lh_g2& g2, const lh_g2& s_g2);
void ukzg_vp_export(const UkzgVerifierParams&, lh_g1* g1, lh_g2* g2, lh_g2* s_g2);
void ukzg_vp_free(UkzgVerifierParams*);
void ukzg_verify(const UkzgVerifierParams&, const HG1& comm, const HFr& point, const HFr& eval, Transcript& tr);
void ukzg_batch_verify(const UkzgVerifierParams&, const HG1* comms, size_t num_comms, const HFr* points, size_t num_points,
                       const lh_evaluation* evals, size_t num_evals, Transcript& tr);
void gemini_verify(const UkzgVerifierParams&, const HG1& comm, const HFr* point, size_t num_vars, const HFr& eval,
                   Transcript& tr);
void gemini_batch_verify(const UkzgVerifierParams&, size_t num_vars, const HG1* comms, size_t num_comms, const HFr* points,
                         size_t num_points, const lh_evaluation* evals, size_t num_evals, Transcript& tr);
PcsVerifier gemini_verifier(const UkzgVerifierParams&);

// ------------------------------------------------------------------ pcs::multilinear::ipa over bn256::G1Affine (ipa.cpp;
// verifier in verifier.cpp).  MultilinearIpaParams (ipa.rs:25-44) is prover and verifier param at once: g on the device
// when set up with a ctx, on the host when not (or on first use by a verifier); `poly_size` is the trim size (a prefix of g).
struct IpaParams {
  size_t num_vars = 0;
  DevMem d_g;
  HG1 h;
  mutable std::vector<HG1> host_g;  // through ipa_host_g
  mutable std::mutex mu;
  // window tables of prefixes of g for the row kernels (dev.hpp k_g1_rows_msm): key = row_len, entry w row_len + i =
  // 2^(8 w) g[i], w < 32; built on first use (ipa.cpp ipa_rows_table), freed with the param
  mutable std::map<size_t, DevMem> rows_tables;
};
HG1 ipa_hash_to_point(const uint8_t* message, size_t len);
std::unique_ptr<IpaParams> ipa_setup(Ctx* c, size_t poly_size);  // c null: host only
const std::vector<HG1>& ipa_host_g(const IpaParams&);
const G1Affine* ipa_rows_table(Ctx&, const IpaParams&, size_t row_len);  // the window table of g[0 .. row_len) (ipa.cpp)
size_t ipa_trim_vars(const IpaParams&, size_t poly_size);   // ipa.rs:129-145 -> num_vars of the trimmed param
std::vector<HG1> ipa_batch_commit(Ctx&, const IpaParams&, size_t poly_size, const Fr* const* d_polys, size_t num_polys,
                                  size_t num_vars);
void ipa_open(Ctx&, const IpaParams&, size_t poly_size, const Fr* d_poly, size_t num_vars, const HFr* point, Transcript& tr);
void ipa_batch_open(Ctx&, const IpaParams&, size_t poly_size, size_t num_vars, const Fr* const* d_polys, size_t num_polys,
                    const HFr* points, size_t num_points, const lh_evaluation* evals, size_t num_evals, Transcript& tr,
                    const SmallPoly* small = nullptr);
// variable_base_msm on the host (bucket method, windows over the host pool): the IPA verifier's 2 n + 2^n + 1 terms
HG1 host_msm(const HFr* scalars, const HG1* bases, size_t n);
void ipa_verify(const IpaParams&, size_t poly_size, const HG1& comm, const HFr* point, size_t num_vars, const HFr& eval,
                Transcript& tr);
void ipa_batch_verify(const IpaParams&, size_t poly_size, size_t num_vars, const HG1* comms, size_t num_comms, const HFr* points,
                      size_t num_points, const lh_evaluation* evals, size_t num_evals, Transcript& tr);
PcsVerifier ipa_verifier(const IpaParams&, size_t poly_size);

// pcs::multilinear::hyrax on top of it (hyrax.rs:23-321): a table of 2^num_vars entries as 2^(num_vars - row_num_vars) rows of
// 2^row_num_vars, one IPA commitment per row; MultilinearHyraxParams = these dimensions + an IpaParams of 2^row_num_vars.
// A commitment is a VECTOR of num_chunks points: Pcs::chunks (hyrax_pcs below).
struct HyraxDims {
  size_t num_vars = 0, batch_num_vars = 0, row_num_vars = 0;
  size_t num_chunks() const { return (size_t)1 << (num_vars - row_num_vars); }
};
HyraxDims hyrax_dims(size_t poly_size, size_t batch_size);                        // hyrax.rs:121-127 (asserts: LH_ERR_ARG)
HyraxDims hyrax_trim(const IpaParams&, size_t poly_size, size_t batch_size);      // hyrax.rs:139-167
// -> num_polys x num_chunks points, poly-major, rows in order (hyrax.rs:199-220)
std::vector<HG1> hyrax_batch_commit(Ctx&, const IpaParams&, size_t poly_size, size_t batch_size, const Fr* const* d_polys,
                                    size_t num_polys, size_t num_vars);
void hyrax_open(Ctx&, const IpaParams&, size_t poly_size, size_t batch_size, const Fr* d_poly, size_t num_vars, const HFr* point,
                Transcript& tr);
void hyrax_batch_open(Ctx&, const IpaParams&, size_t poly_size, size_t batch_size, size_t num_vars, const Fr* const* d_polys,
                      size_t num_polys, const HFr* points, size_t num_points, const lh_evaluation* evals, size_t num_evals,
                      Transcript& tr, const SmallPoly* small = nullptr);
void hyrax_verify(const IpaParams&, size_t poly_size, size_t batch_size, const HG1* comm, const HFr* point, size_t num_vars,
                  const HFr& eval, Transcript& tr);
void hyrax_batch_verify(const IpaParams&, size_t poly_size, size_t batch_size, size_t num_vars, const HG1* comms, size_t num_comms,
                        const HFr* points, size_t num_points, const lh_evaluation* evals, size_t num_evals, Transcript& tr);
PcsVerifier hyrax_verifier(const IpaParams&, size_t poly_size, size_t batch_size);  // chunks from hyrax_trim

// what the provers (Lasso, HyperPlonk and its Lasso lookups) need from their PCS: the PolynomialCommitmentScheme the
// backend is generic over (backend/hyperplonk.rs:76-95), plus the bases themselves for the small-valued Lasso columns
// a column for Pcs::commit_columns: `len` <= 2^nv entries, Fr (Montgomery) or u32 with every value < 2^known_bits (1..32),
// committed as the table zero-padded to nv variables
struct PcsColumn {
  const void* data;
  bool u32;
  size_t len;
  uint32_t known_bits;
};
struct Pcs {
  // points per commitment (Hyrax: its num_chunks row commitments); batch_commit returns num_polys * chunks points,
  // poly-major, rows in order - what the scheme's batch_commit_and_write writes
  size_t chunks = 1;
  std::function<std::vector<HG1>(const Fr* const* d_polys, size_t num_polys, size_t num_vars)> batch_commit;
  // optional (a scheme whose commitment is not a vector of points - Brakedown: device-resident rows and a Merkle tree):
  // commits the polys and writes the commitments itself, used in place of batch_commit + Transcript::write_commitments;
  // the scheme keeps what it committed and its batch_open finds the commitment of an opened poly by its device pointer
  std::function<void(const Fr* const* d_polys, size_t num_polys, size_t num_vars, Transcript& tr)> commit_and_write;
  // optional (schemes without commit_bases: Hyrax): commits (small-valued) columns directly -> num_cols * chunks points
  std::function<std::vector<HG1>(const PcsColumn* cols, size_t num_cols, size_t nv)> commit_columns;
  // optional (Brakedown): commit_columns as commit_and_write is to batch_commit - commits the columns as one batch (columns
  // that share a data pointer once), writes one commitment per column itself and keeps them; its batch_open finds a
  // column's commitment by the column's device pointer (SmallPoly::ptr, or the table's where there is no u32 form)
  std::function<void(const PcsColumn* cols, size_t num_cols, size_t nv, Transcript& tr)> commit_columns_and_write;
  // bases whose first 2^nv points commit a zero-padded table of 2^nv entries (the eq basis of level nv, or the powers of
  // s): the small-valued Lasso columns are committed as u32 MSMs against them.  nv <= max_vars is the caller's check
  // (LH_ERR_INVALID_PCS_PARAM, "Too many variates of poly to commit")
  std::function<const G1Affine*(size_t nv)> commit_bases;
  // one proof over several GPUs (dev.hpp Shard): this rank's share of commit_bases; batch_commit / batch_open then take
  // this rank's shards and add the ranks' partial commitments (null: this PCS does not shard)
  std::function<const G1Affine*(size_t nv)> shard_bases;
  size_t max_vars = 0;
  // small (null allowed): the polys that came as small-valued u32 columns (SmallPoly above)
  std::function<void(size_t num_vars, const Fr* const* d_polys, size_t num_polys, const HFr* points, size_t num_points,
                     const lh_evaluation* evals, size_t num_evals, Transcript& tr, const SmallPoly* small)>
      batch_open;
  // optional (multilinear KZG): start committing the challenge-free half of that batch opening now (open_precommit_start;
  // `staged` as there, -1: all of it now)
  std::function<bool(size_t num_vars, const SmallPoly* small, size_t num_polys, const lh_evaluation* evals, size_t num_evals,
                     int staged)>
      precommit;
};
Pcs mkzg_pcs(Ctx&, const Srs&);                            // mkzg.cpp
Pcs zeromorph_pcs(Ctx&, const USrs&, size_t poly_size);    // zeromorph.cpp
Pcs gemini_pcs(Ctx&, const USrs&, size_t poly_size);       // gemini.cpp
Pcs ipa_pcs(Ctx&, const IpaParams&, size_t poly_size);     // ipa.cpp (no shard_bases, no precommit)
// ipa.cpp: commitments of num_chunks points, commit_columns instead of commit_bases; commits only polys of exactly
// log2(poly_size) variables (LH_ERR_ARG otherwise)
Pcs hyrax_pcs(Ctx&, const IpaParams&, size_t poly_size, size_t batch_size);
// (brakedown_pcs: brakedown.hpp - it needs the hash transcript and the commitments of the polys the caller committed)

// ------------------------------------------------------------------ steps shared by the arguments (argument.cpp)
// What Lasso, LogUp-GKR, memory checking and Spark all do, defined once; a new argument starts from these.
// bit length of v (0 for 0); a width that must be at least one bit says std::max(bit_length(v), 1u)
inline uint32_t bit_length(uint64_t v) { return v ? 64u - (uint32_t)__builtin_clzll(v) : 0u; }
// one entry of an opening list: poly `poly` at point `point` is *value (null: zero, to be filled in later)
inline lh_evaluation make_evaluation(size_t poly, size_t point, const HFr* value) {
  lh_evaluation e;
  memset(&e, 0, sizeof(e));
  e.poly = (uint32_t)poly, e.point = (uint32_t)point;
  if (value) memcpy(&e.value, value, 32);
  return e;
}
// The refusals of the stand-alone argument `name` (the prefix of every message).  Prover: no sharded proofs; a scheme whose
// commitment is one point over bases (batch_commit too where the argument commits field-element tables) that reaches nv
// variables.  Verifier: commitments of one point.
void argument_not_sharded(Ctx&, const std::string& name);
void argument_pcs_check(const Pcs&, size_t nv, const std::string& name, bool needs_batch_commit);
void argument_pcs_check(const PcsVerifier&, const std::string& name);
// Commits u32 columns of their own lengths, each a 32-bit MSM against the bases of level nv (zero-padding is implicit) whose
// width max(bit_length(OR of its entries), 1) is promised to the MSM: ONE k_or_u32 per distinct length over the columns
// whose OR the caller does not hold already (known_or), ONE msm_batch.  -> the points; bits[k]: column k's width, which the
// opening is promised too (SmallPoly::bits).  A width that differs between the two gives a wrong commitment: THE rule is here.
struct U32Column {
  const uint32_t* ptr;
  size_t len;
  const uint32_t* known_or = nullptr;
};
std::vector<HG1> commit_u32_columns(Ctx&, const Pcs&, size_t nv, const std::vector<U32Column>& cols, uint32_t* bits);
// u32 columns of 2^vars entries evaluated at `point`, against its full eq table (scratch of this call)
void evaluate_u32_columns(Ctx&, const uint32_t* const* cols, size_t count, const HFr* point, size_t vars, HFr* out);
// The four product trees per memory of ONE grand-product GKR over A memories: RS, WS of memory b (n variables) at 2 b and
// 2 b + 1, behind them Init, Final (l variables) at 2 A + 2 b and 2 A + 2 b + 1.  ws_plus_one (Lasso, Spark): write leaf =
// read leaf + 1: where the n-variable trees are alone at their leaf layer that layer runs over the read-set tables only
// (prove_grand_product: plus_one) and the write-set leaves are never stored (ws_implicit).  The caller fills the leaves.
struct MemoryTrees {
  size_t A;
  bool ws_plus_one;
  std::vector<const Fr*> leaves, level_up;
  std::vector<size_t> depths;
  std::vector<uint8_t> plus_one;
  MemoryTrees(size_t A_, size_t n, bool ws_plus_one_ = true)
      : A(A_), ws_plus_one(ws_plus_one_), leaves(4 * A_), level_up(4 * A_, nullptr), depths(4 * A_, n), plus_one(4 * A_, 0) {}
  struct Memory {
    Fr *rs, *ws, *rs_up, *ws_up, *init, *fin, *init_up, *fin_up;
  };
  // memory b's leaf tables (N and M = 2^l entries; up_n / up_l: the level above the n- / l-variable leaves comes with them)
  Memory add(Ctx& c, size_t b, size_t N, size_t l, bool up_n, bool ws_implicit, bool up_l = false);
  GrandProductResult prove(Ctx& c, Transcript& tr, const std::function<void()>& trees_built = nullptr) {
    return prove_grand_product(c, 4 * A, leaves.data(), depths.data(), tr, level_up.data(), ws_plus_one ? plus_one.data() : nullptr,
                               trees_built);
  }
};
// the verifiers' side of those trees: the fingerprint h(a, v, t) = a gamma^2 + v gamma + t - tau of a memory operation
struct Fingerprint {
  HFr gamma, tau;
  HFr operator()(const HFr& a, const HFr& v, const HFr& t) const { return a * gamma * gamma + v * gamma + t - tau; }
};
// the LogUp identity on the roots of two fractions: P_0 / Q_0 + P_1 / Q_1 = 0 with both denominators non-zero
inline bool logup_roots_cancel(const HFr& p0, const HFr& q0, const HFr& p1, const HFr& q1) {
  return !q0.is_zero() && !q1.is_zero() && (p0 * q1 + p1 * q0).is_zero();
}
// the multilinear extension at x (variable i = index bit i) of a host table of 2^l rows, row(r) its entry r: one fold over
// the rows (the first, which reads them, over the host pool)
HFr host_table_eval(size_t l, const std::vector<HFr>& x, const std::function<HFr(size_t)>& row);
// The verdict of a verifier entry: a proof that does not verify is LH_ERR_INVALID_SNARK whichever piece found it out (a round
// message, an opening, bytes that are no point or no field element, a proof that ends early): the message keeps the piece's
// own words behind "<name>: ".  What is wrong with the call, not with the proof, keeps its code (LH_ERR_ARG,
// LH_ERR_INVALID_PCS_PARAM).
void argument_verdict(const std::string& name, const std::function<void()>& verify);
// A commitment blob - a transcript's stream of its own: the mask element, then the non-identity points, nothing else - read
// back as `count` commitments; malformed: LH_ERR_INVALID_SNARK "<name>: malformed commitment: ..."
std::vector<HG1> argument_read_commitment_blob(const std::string& name, const uint8_t* blob, size_t len, size_t count);
// commitments that are part of a statement: the mask element (bit i: commitment i is the identity), then the other points
void argument_absorb_commitments(Transcript& tr, const std::vector<HG1>& comms);

// ------------------------------------------------------------------ Lasso
// pieces of the argument shared by the standalone prover (lasso.cpp) and HyperPlonk's Lasso lookups (hyperplonk.cpp)
struct SubtableOrders;
struct LassoColumns {  // small-valued witness columns as u32 (arena memory of the caller's scope)
  std::vector<uint32_t*> rts, fcs, E;
  std::vector<const uint32_t*> T;  // per memory: the device entries of a registered subtable (null: a built-in kind)
  std::shared_ptr<SubtableOrders> tables;  // owner of those (and of the derived commitments' orders); one upload per kind
  std::vector<uint32_t*> dim_sorted, dim_index;  // (keep_sorted) every dim column sorted by value + source positions
  uint32_t a_bits = 0;  // a 32-bit output column of a product g: every entry < 2^a_bits (0: none, or the linear g's column)
};
struct LassoClaims {  // points and claimed evaluations that remain to be opened
  std::vector<HFr> r, r_z, r_N, r_M;
  HFr v;                  // a(r)
  std::vector<HFr> e_rz;  // E_i(r_z)
  std::vector<HFr> ev_n;  // dim_j | read_ts_j | E_i at r_N
  std::vector<HFr> ev_l;  // final_cts_j at r_M
};
// One table's shape and THE proof layout: the positions of its committed polys inside its commitment block,
// a | dim_j | read_ts_j | E_i | final_cts_j.  Every prover, verifier and opening list takes its positions from here.
struct LassoLayout {
  size_t cc = 0, l = 0, alpha = 0;
  bool linear_g = true;  // every term of g has one factor (range / AND / XOR / OR): a = sum_m coeff_m E_f(m) entry by entry
  size_t g_degree = 0;   // the most factors in a term of g
  LassoLayout() = default;
  explicit LassoLayout(const lh_lasso_table& tb) : cc(tb.num_chunks), l(tb.chunk_bits), alpha(tb.num_memories) {
    // (a table nobody has validated yet may be handed in - HyperPlonk counts its commitments before it checks its lookups:
    // no read past the arrays; lasso_check_table refuses such a term count)
    for (uint32_t m = 0; m < tb.num_terms && m < LH_LASSO_MAX_TERMS; m++) {
      linear_g = linear_g && tb.g_num_factors[m] == 1;
      g_degree = std::max<size_t>(g_degree, tb.g_num_factors[m]);
    }
  }
  size_t a() const { return 0; }
  size_t dim(size_t j) const { return 1 + j; }
  size_t read_ts(size_t j) const { return 1 + cc + j; }
  size_t E(size_t i) const { return 1 + 2 * cc + i; }
  size_t final_cts(size_t j) const { return 1 + 2 * cc + alpha + j; }
  size_t num_polys() const { return 1 + 3 * cc + alpha; }
  size_t num_at_n() const { return 2 * cc + alpha; }  // the evaluations at r_N: dim_j | read_ts_j | E_i (LassoClaims::ev_n)
};
// Where a table's polys and points sit in a batch opening: the poly index of a, of every dim_j, and of the first read_ts, E
// and final_cts (each group consecutive); the point indices of r, r_z, r_N, r_M.
struct LassoOpening {
  size_t a = 0;
  std::vector<size_t> dim;
  size_t read_ts = 0, E = 0, final_cts = 0;
  size_t r = 0, r_z = 1, r_N = 2, r_M = 3;
  // a commitment block of the layout's own at poly `poly_base`; points 0, 1, 2 and `r_M`
  static LassoOpening block(const LassoLayout& lay, size_t poly_base = 0, size_t r_M = 3) {
    LassoOpening o;
    o.a = poly_base + lay.a(), o.read_ts = poly_base + lay.read_ts(0), o.E = poly_base + lay.E(0), o.final_cts = poly_base + lay.final_cts(0);
    for (size_t j = 0; j < lay.cc; j++) o.dim.push_back(poly_base + lay.dim(j));
    o.r_M = r_M;
    return o;
  }
  // a lookup of a HyperPlonk circuit: a and dim_j are circuit polys, read_ts | E | final_cts start at `base`; points from p0
  static LassoOpening in_circuit(const LassoLayout& lay, size_t output_poly, const size_t* chunk_polys, size_t base, size_t p0) {
    LassoOpening o;
    o.a = output_poly, o.dim.assign(chunk_polys, chunk_polys + lay.cc);
    o.read_ts = base, o.E = base + lay.cc, o.final_cts = base + lay.cc + lay.alpha;
    o.r = p0, o.r_z = p0 + 1, o.r_N = p0 + 2, o.r_M = p0 + 3;
    return o;
  }
  static size_t circuit_polys(const LassoLayout& lay) { return lay.num_polys() - 1 - lay.cc; }  // read_ts | E | final_cts
};
// THE opening list of a Lasso argument, walked once: a at r; E_i at r_z; dim_j | read_ts_j | E_i at r_N; final_cts_j at r_M.
// f(poly, point, value) per entry; value is null without claims (the pairs alone, before the challenges exist).
template <class F>
inline void lasso_opening_walk(const LassoLayout& lay, const LassoOpening& o, const LassoClaims* cl, F&& f) {
  auto at = [&](const std::vector<HFr> LassoClaims::*group, size_t k) { return cl ? &(cl->*group)[k] : nullptr; };
  f(o.a, o.r, cl ? &cl->v : nullptr);
  for (size_t i = 0; i < lay.alpha; i++) f(o.E + i, o.r_z, at(&LassoClaims::e_rz, i));
  for (size_t j = 0; j < lay.cc; j++) f(o.dim[j], o.r_N, at(&LassoClaims::ev_n, j));
  for (size_t j = 0; j < lay.cc; j++) f(o.read_ts + j, o.r_N, at(&LassoClaims::ev_n, lay.cc + j));
  for (size_t i = 0; i < lay.alpha; i++) f(o.E + i, o.r_N, at(&LassoClaims::ev_n, 2 * lay.cc + i));
  for (size_t j = 0; j < lay.cc; j++) f(o.final_cts + j, o.r_M, at(&LassoClaims::ev_l, j));
}
// the list appended to `evs`, with the values of `cl` or (null) zeros that lasso_evaluation_values fills later
inline void lasso_evaluation_list(const LassoLayout& lay, const LassoOpening& o, const LassoClaims* cl, std::vector<lh_evaluation>& evs) {
  lasso_opening_walk(lay, o, cl, [&](size_t poly, size_t point, const HFr* val) { evs.push_back(make_evaluation(poly, point, val)); });
}
// the values of a list made without claims, in place: the same walk
inline void lasso_evaluation_values(const LassoLayout& lay, const LassoOpening& o, const LassoClaims& cl, lh_evaluation* evs) {
  lasso_opening_walk(lay, o, &cl, [&](size_t, size_t, const HFr* val) { memcpy(&(evs++)->value, val, 32); });
}
// the points of the argument join those of a batch opening over nv variables, each zero-padded
inline void lasso_append_points(std::vector<HFr>& points, const std::vector<const std::vector<HFr>*>& pts, size_t nv) {
  for (const std::vector<HFr>* pt : pts) {
    points.insert(points.end(), pt->begin(), pt->end());
    points.insert(points.end(), nv - pt->size(), HFr::zero());
  }
}
// term m's coefficient of g; whether it is an integer below 2^bits (bits <= 64; *low: that integer)
inline HFr lasso_g_coeff(const lh_lasso_table& tb, size_t m) {
  HFr co;
  memcpy(&co, &tb.g_coeff[m], 32);
  return co;
}
inline bool lasso_g_coeff_fits(const lh_lasso_table& tb, size_t m, unsigned bits, uint64_t* low = nullptr) {
  uint64_t canon[4];
  lasso_g_coeff(tb, m).to_canonical(canon);
  if (low) *low = canon[0];
  return !canon[1] && !canon[2] && !canon[3] && (bits >= 64 || !(canon[0] >> bits));
}
constexpr uint32_t LH_SUBTABLE_KINDS = 6;  // IDENTITY .. LTU (include/lasso_hip.h)
// Caller-registered subtables (subtable.cpp; include/lasso_hip.h lh_subtable_register): kinds from LH_SUBTABLE_CUSTOM_BASE up.
// Immutable once registered; the shared_ptr of a lookup keeps the entries alive past an unregister on another thread.
struct CustomSubtable {
  uint32_t kind = 0, chunk_bits = 0, value_bits = 0;  // value_bits: bit length of the largest entry (0: all zero)
  uint8_t digest[32] = {0};                           // Keccak-256 of the entries as little-endian words
  std::vector<uint32_t> values;                       // 2^chunk_bits entries
  std::vector<uint32_t> order;                        // T[0] = 0 only: the indices sorted by entry (MsmJob::d_order)
};
uint32_t subtable_register(const uint32_t* values, uint32_t chunk_bits);
void subtable_unregister(uint32_t kind);
std::shared_ptr<const CustomSubtable> subtable_find(uint32_t kind);  // null: not registered
// the registered subtable a memory of a table of 2^l-entry chunks names: LH_ERR_ARG when there is none or its size differs
std::shared_ptr<const CustomSubtable> subtable_require(uint32_t kind, size_t l);
inline bool subtable_is_custom(uint32_t kind) { return kind >= LH_SUBTABLE_CUSTOM_BASE; }
// THE width rule: every entry of a subtable of 2^l entries is below 2^lasso_subtable_bits(kind, l).  What is promised to
// the u32 MSM and the column commits (known_bits) comes from here: a bound too small yields wrong commitments.
inline uint32_t lasso_subtable_bits(uint32_t kind, size_t l) {
  if (subtable_is_custom(kind)) return subtable_require(kind, l)->value_bits;  // (0: an all-zero table)
  if (kind == LH_SUBTABLE_IDENTITY) return (uint32_t)l;
  if (kind == LH_SUBTABLE_EQ || kind == LH_SUBTABLE_LTU) return 1;
  return (uint32_t)(l / 2);  // AND, XOR, OR of two (l / 2)-bit halves
}
// entry m = x || y (y: the low l / 2 bits) of a non-identity subtable - the host's copy of kernels_poly.hip subtable_entry
inline uint32_t lasso_subtable_entry_host(uint32_t kind, uint32_t m, size_t l) {
  const size_t h = l / 2;
  const uint32_t x = m >> h, y = m & (((uint32_t)1 << h) - 1u);
  switch (kind) {
    case LH_SUBTABLE_AND: return x & y;
    case LH_SUBTABLE_XOR: return x ^ y;
    case LH_SUBTABLE_OR: return x | y;
    case LH_SUBTABLE_EQ: return x == y ? 1u : 0u;
    case LH_SUBTABLE_LTU: return x < y ? 1u : 0u;
    default: return m;
  }
}
// T[d] and the d's sorted by T[d] for the non-identity subtables, on the device (arena memory of the caller's scope; the
// host staging lives as long as this object, i.e. past the msm_batch that consumes them).  A registered kind is served
// from the registry's entries, which this object keeps alive; its device T is what the witness and leaf kernels gather from.
struct SubtableOrders {
  struct Entry {
    std::vector<uint32_t> h_tab, h_ord;
    std::shared_ptr<const CustomSubtable> custom;
    uint32_t *d_tab = nullptr, *d_ord = nullptr;
  };
  Ctx& c;
  size_t l;
  std::map<uint32_t, Entry> entries;  // one per distinct kind
  SubtableOrders(Ctx& c_, size_t l_) : c(c_), l(l_) {}
  // T of a registered kind alone (one upload per kind); its first entry: *t0
  const uint32_t* custom_table(uint32_t kind, uint32_t* t0 = nullptr) {
    Entry& e = entries[kind];
    if (!e.d_tab) {
      e.custom = subtable_require(kind, l);
      const size_t M = (size_t)1 << l;
      e.d_tab = c.arena.alloc_n<uint32_t>(M);
      LH_HIP(hipMemcpyAsync(e.d_tab, e.custom->values.data(), M * 4, hipMemcpyHostToDevice, c.stream));
    }
    if (t0) *t0 = e.custom->values[0];
    return e.d_tab;
  }
  void get(uint32_t kind, const uint32_t** table, const uint32_t** order) {
    const size_t M = (size_t)1 << l;
    if (subtable_is_custom(kind)) {
      *table = custom_table(kind);
      Entry& e = entries[kind];
      if (!e.d_ord) {
        // (sorted by entry once, at registration: 32-bit values rule out the counting sort below)
        LH_REQUIRE(e.custom->order.size() == M, LH_ERR_ARG, "lasso: a derived commitment needs T[0] = 0");
        e.d_ord = c.arena.alloc_n<uint32_t>(M);
        LH_HIP(hipMemcpyAsync(e.d_ord, e.custom->order.data(), M * 4, hipMemcpyHostToDevice, c.stream));
      }
      *order = e.d_ord;
      return;
    }
    LH_REQUIRE(kind > LH_SUBTABLE_IDENTITY && kind < LH_SUBTABLE_KINDS, LH_ERR_ARG, "lasso: unknown subtable");
    Entry& e = entries[kind];
    if (!e.d_tab) {
      const size_t V = (size_t)1 << lasso_subtable_bits(kind, l);
      std::vector<uint32_t>&tab = e.h_tab, &ord = e.h_ord;
      tab.resize(M), ord.resize(M);
      std::vector<uint32_t> start(V + 1, 0);
      for (size_t d = 0; d < M; d++) {
        tab[d] = lasso_subtable_entry_host(kind, (uint32_t)d, l);
        start[tab[d] + 1]++;
      }
      for (size_t v = 0; v < V; v++) start[v + 1] += start[v];
      for (size_t d = 0; d < M; d++) ord[start[tab[d]]++] = (uint32_t)d;  // counting sort by T
      e.d_tab = c.arena.alloc_n<uint32_t>(M);
      e.d_ord = c.arena.alloc_n<uint32_t>(M);
      LH_HIP(hipMemcpyAsync(e.d_tab, tab.data(), M * 4, hipMemcpyHostToDevice, c.stream));
      LH_HIP(hipMemcpyAsync(e.d_ord, ord.data(), M * 4, hipMemcpyHostToDevice, c.stream));
    }
    *table = e.d_tab, *order = e.d_ord;
  }
};

void lasso_check_table(const lh_lasso_table& tb);
// a_out (optional): the output column a = g(E) as field elements; a_small_out (optional): the same as a 32-bit column
// when g is linear with small coefficients and the value fits, or has product terms whose bound fits (LassoColumns::a_bits;
// then *a_out stays null); reuse (optional; rts / fcs sized num_chunks): a non-null rts[j] / fcs[j] pair is taken for chunk j
// instead of counting the column again (a batch whose tables share chunk columns)
LassoColumns lasso_witness_columns(Ctx&, const lh_lasso_table&, size_t n, const uint32_t* const* d_dims, Fr** a_out,
                                   uint32_t** a_small_out = nullptr, bool keep_sorted = false,
                                   const LassoColumns* reuse = nullptr);
// `a`: the output column as field elements, or null with `a_small` given
LassoClaims lasso_argue(Ctx&, const lh_lasso_table&, size_t n, const LassoColumns& w, const uint32_t* const* d_dims,
                        const Fr* a, const Fr* const* E_fr, Transcript& tr,
                        const std::function<void(int)>& lap = nullptr, const uint32_t* a_small = nullptr,
                        const std::function<void()>& trees_built = nullptr);
// commitment framing of the Lasso argument: identity masks (one field element per 63 points of the count * chunks points,
// flattened commitment-major), then the non-identity points
void lasso_write_commitments(Transcript& tr, const std::vector<HG1>& comms, size_t chunks = 1);
std::vector<HG1> lasso_read_commitments(Transcript& tr, size_t count, size_t chunks = 1);
void lasso_prove(Ctx&, const Pcs&, const lh_lasso_table& table, size_t num_vars, const uint32_t* const* d_dims,
                 Transcript& tr);
// Lookups into several tables (the same number of lookups each) in ONE proof: one commit batch, one Surge sum-check, one
// grand-product GKR, one batch opening (tests/lasso_batch_ref.py).  d_dims[t][j]: chunk column j of table t.
// lasso_batch_check: the limits of a batch that need no device (shared with the verifier); returns nv = max(n, max l_t)
size_t lasso_batch_check(const lh_lasso_table* const* tables, size_t num_tables, size_t num_vars);
void lasso_prove_batch(Ctx&, const Pcs&, const lh_lasso_table* const* tables, size_t num_tables, size_t num_vars,
                       const uint32_t* const* const* d_dims, Transcript& tr);

// ------------------------------------------------------------------ LogUp-GKR (logup.cpp; tests/logup_gkr_ref.py)
// the limits that need no device (shared with the verifier, which has no input columns): returns nv = max(n, l)
size_t logup_check(const lh_logup_lookup* lookups, size_t num_lookups, size_t num_vars, size_t table_vars, bool prover);
void logup_gkr_prove(Ctx&, const Pcs&, const lh_logup_lookup* lookups, size_t num_lookups, size_t num_vars, size_t table_vars,
                     Transcript& tr);
// the same prover over columns of either kind (lh_logup_columns: some input columns are uint32_t); the entry above is this one
// with every kind LH_LOGUP_COL_FR
void logup_gkr_prove_columns(Ctx&, const Pcs&, const lh_logup_columns* lookups, size_t num_lookups, size_t num_vars,
                             size_t table_vars, Transcript& tr);
void logup_gkr_verify(const PcsVerifier& pcs, const lh_logup_lookup* lookups, size_t num_lookups, size_t num_vars,
                      size_t table_vars, Transcript& tr);

// ------------------------------------------------------------------ read-write memory checking (memcheck.cpp; tests/memcheck_ref.py)
// the limits that need no device (shared with the verifier): returns nv = max(num_vars, mem_vars)
size_t memcheck_check(size_t num_vars, size_t mem_vars, bool has_init);
// trace: three device u32 columns of 2^num_vars entries; init: HOST, 2^mem_vars words, or null for an all-zero image
void memcheck_prove(Ctx&, const Pcs&, const lh_memcheck_trace& trace, size_t num_vars, size_t mem_vars, const uint32_t* init,
                    Transcript& tr);
void memcheck_verify(const PcsVerifier& pcs, size_t num_vars, size_t mem_vars, const uint32_t* init, Transcript& tr);
// the witness kernels alone (lh_debug_memcheck_witness): false when the trace is invalid
bool memcheck_witness(Ctx&, const lh_memcheck_trace& trace, size_t num_vars, size_t mem_vars, const uint32_t* init, uint32_t* d_rt,
                      uint32_t* d_fv, uint32_t* d_ft, uint32_t* d_m);
// the trace's rv and wv (and the final cells; null: not wanted) from the operations, on the device; d_image null: all zero
void memcheck_replay(Ctx&, const lh_memcheck_ops& ops, size_t num_vars, size_t mem_vars, const uint32_t* d_image, uint32_t* d_rv,
                     uint32_t* d_wv, uint32_t* d_final);
// Segment proofs (tests/memcheck_segment_ref.py): the image a committed DEVICE column, never null; d_final (device, or null)
// receives the final values - the next segment's image.  The verifier returns the commitments of image and final values.
size_t memcheck_segment_check(size_t num_vars, size_t mem_vars);
void memcheck_prove_segment(Ctx&, const Pcs&, const lh_memcheck_trace& trace, size_t num_vars, size_t mem_vars,
                            const uint32_t* d_image, uint32_t* d_final, Transcript& tr);
void memcheck_verify_segment(const PcsVerifier& pcs, size_t num_vars, size_t mem_vars, Transcript& tr, HG1* image_commitment,
                             HG1* final_commitment);

// ------------------------------------------------------------------ Spark (spark.cpp; tests/spark_ref.py)
// A committed sparse polynomial: 2^n entries (dim_0 .. dim_{c-1}, val) with indices below 2^l.  Owns ONE device block outside
// the arena - copies of the index columns, val zero-padded to nv = max(n, l) variables, the access counters - and the
// commitments of [val | dim_j | read_ts_j | final_cts_j]; listed in Ctx::spark_polys until spark_free or the ctx's end.
struct SparkPoly {
  Ctx* ctx = nullptr;
  size_t n = 0, l = 0, c = 0, nv = 0;
  DevMem block;
  const Fr* val = nullptr;  // 2^nv entries
  const uint32_t *dim[SPARK_MAX_DIMS] = {}, *rts[SPARK_MAX_DIMS] = {}, *fcs[SPARK_MAX_DIMS] = {};  // 2^n, 2^n, 2^l entries
  uint32_t dim_bits[SPARK_MAX_DIMS] = {}, rts_bits[SPARK_MAX_DIMS] = {}, fcs_bits[SPARK_MAX_DIMS] = {};  // widths (>= 1)
  std::vector<HG1> comms;     // 1 + 3 c, commitment order
  std::vector<uint8_t> blob;  // lasso_write_commitments of them on a fresh transcript: the mask element, the points
};
// the limits that need no device (shared with the verifier): returns nv = max(num_vars, dim_vars)
size_t spark_check(size_t num_vars, size_t dim_vars, size_t num_dims);
SparkPoly* spark_commit(Ctx&, const Pcs&, size_t num_vars, size_t dim_vars, size_t num_dims, const uint32_t* const* d_dims,
                        const Fr* d_val);
void spark_free(Ctx&, SparkPoly*);  // (not one of this ctx's: nothing happens)
void spark_free_all(Ctx&);
// point: num_dims * dim_vars coordinates; appends the proof, returns the value
HFr spark_open(Ctx&, const Pcs&, const SparkPoly&, const HFr* point, Transcript& tr);
void spark_verify(const PcsVerifier& pcs, size_t num_vars, size_t dim_vars, size_t num_dims, const uint8_t* commitment,
                  size_t commitment_len, const HFr* point, const HFr& value, Transcript& tr);
// the memory kernel alone (lh_debug_spark_e)
HFr spark_debug_e(Ctx&, size_t num_vars, size_t dim_vars, size_t num_dims, const uint32_t* const* d_dims, const Fr* d_val,
                  const HFr* point, Fr* const* d_E);

// ------------------------------------------------------------------ Spartan (spartan.cpp; tests/spartan_ref.py)
// The key of an R1CS instance: the Spark commitments of A, B, C (ordinary polynomials of this ctx: spark_open takes them) and,
// per matrix and direction (0: by rows, 1: by columns), the entry stream sorted by that index - the sorted keys, the other
// index permuted along, the position of every entry's value - in ONE device block outside the arena (18 * 2^n words): a
// prove runs no sort.  Listed in Ctx::r1cs_keys until spartan_free or the ctx's end.
struct R1csKey {
  Ctx* ctx = nullptr;
  size_t n = 0, l = 0;
  SparkPoly* mat[3] = {};  // freed with the key
  DevMem block;
  const uint32_t *seg[2][3] = {}, *other[2][3] = {}, *perm[2][3] = {};
  std::vector<uint8_t> blob;  // the three commitment blobs one after the other
  ~R1csKey();
};
// the limits that need no device (shared with the verifier): returns max(num_vars, dim_vars)
size_t spartan_check(size_t num_vars, size_t dim_vars, size_t num_public);
R1csKey* spartan_commit(Ctx&, const Pcs&, size_t num_vars, size_t dim_vars, const lh_r1cs_matrix* m);
void spartan_free(Ctx&, R1csKey*);  // (not one of this ctx's: nothing happens)
void spartan_free_all(Ctx&);
// d_w: 2^(dim_vars - 1) device field elements; x: num_public host ones; appends the proof
void spartan_prove(Ctx&, const Pcs&, const R1csKey&, const Fr* d_w, const HFr* x, size_t num_public, Transcript& tr);
void spartan_verify(const PcsVerifier& pcs, size_t num_vars, size_t dim_vars, const uint8_t* key, size_t key_len, const HFr* x,
                    size_t num_public, Transcript& tr);
// the keyed-sum kernel alone (lh_debug_spartan_spmv): direction 0, d_out[m] = M_m d_x; 1, d_out[m] = M_m^T d_x
void spartan_debug_spmv(Ctx&, const R1csKey&, int direction, const Fr* d_x, Fr* const* d_out);
// The steps the relaxed form and the fold (nova.cpp) take too.  spartan_key_header: n, l, p, then per matrix the commitment's
// mask and its non-identity points; spartan_doubled_evaluation: THE opening list of one poly at one point - batch_open takes at
// least two evaluations (eq_xy of an empty point is the zero poly), so the one evaluation is listed twice: the merged poly is
// ((1 - t) + t) w; spartan_assignment: z = (w, x, 0) of 2^l entries
void spartan_key_header(Transcript& tr, size_t n, size_t l, size_t p, const std::vector<HG1>* comms);
std::vector<lh_evaluation> spartan_doubled_evaluation(const HFr& e);
void spartan_spmv(Ctx&, const R1csKey&, int direction, const Fr* X, Fr* const* out);
void spartan_require_key(Ctx&, const R1csKey&, const char* name);
void spartan_assignment(Ctx&, size_t l, const Fr* d_w, const HFr* x, size_t p, Fr* z);
void spartan_inner_prove(Ctx&, const Pcs&, const R1csKey&, const Fr* z, const Fr* d_w, Fr* const* Mz, const std::vector<HFr>& r_x,
                         const HFr* at_rx, Transcript& tr, std::vector<HFr>& r_y, std::vector<HFr>& e);
void spartan_open_matrices(Ctx&, const Pcs&, const R1csKey&, const std::vector<HFr>& r_x, const std::vector<HFr>& r_y,
                           const std::vector<HFr>& e, Transcript& tr);
struct SpartanKeyBlob {  // the key bytes taken apart: per matrix its commitment blob (into the caller's bytes) and its points
  const uint8_t* blob[3];
  size_t blob_len[3];
  std::vector<HG1> comms[3];
};
SpartanKeyBlob spartan_read_key(const char* name, const uint8_t* key, size_t key_len);  // malformed: LH_ERR_INVALID_SNARK "<name>: malformed key: ..."
void spartan_inner_verify(const PcsVerifier& pcs, size_t l, const HFr* x, size_t p, const HG1& cw, const HFr* v, Transcript& tr,
                          std::vector<HFr>& r_y, std::vector<HFr>& e);
// its two halves, which the batch verifier (spartan_batch.cpp) calls with statements of its own: rho, the inner rounds and
// eA, eB, eC; then e_w, the final claim over the public half x and the opening of the witness (`vars` variables, at `point`)
struct SpartanInnerClaim {
  HFr rho, final;
  std::vector<HFr> r_y, e;
};
SpartanInnerClaim spartan_inner_rounds_verify(size_t l, const HFr* v, Transcript& tr);
void spartan_witness_verify(const PcsVerifier& pcs, const SpartanInnerClaim& claim, size_t l, const HFr* x, size_t p, const HG1& cw,
                            size_t vars, const HFr* point, Transcript& tr);
void spartan_verify_matrices(const PcsVerifier& pcs, size_t n, size_t l, const SpartanKeyBlob& k, const std::vector<HFr>& r_x,
                             const std::vector<HFr>& r_y, const std::vector<HFr>& e, Transcript& tr);

// ------------------------------------------------------------------ batched Spartan, the verifier (spartan_batch.cpp;
// tests/spartan_batch_ref.py): num_instances >= 2 assignments of one key in one proof, batch_vars = ceil(log2 num_instances).
// -> batch_vars; the limits that need no device, after spartan_check's
size_t spartan_batch_check(size_t dim_vars, size_t num_instances);
void spartan_verify_batch(const PcsVerifier& pcs, size_t num_vars, size_t dim_vars, const uint8_t* key, size_t key_len, const HFr* x,
                          size_t num_instances, size_t num_public, Transcript& tr);

// ------------------------------------------------------------------ Nova folding (nova.cpp; tests/nova_ref.py)
// A relaxed instance (C_W, C_E, x), u = x[0], travels as a blob: lasso_write_commitments of [C_W, C_E] on a fresh transcript,
// then the elements of x; its number of public inputs follows from its mask and its length.  Every entry returns the blob it
// makes; `room` is what the caller's buffer takes, checked against LH_NOVA_INSTANCE_BYTES(num_public) before any work.  A blob
// that cannot be read is LH_ERR_ARG at the provers, whose call it is part of, LH_ERR_INVALID_SNARK at the verifiers.
// the fresh instance of a satisfying assignment with x[0] = 1: C_E the identity
std::vector<uint8_t> nova_instance(Ctx&, const Pcs&, const R1csKey&, const Fr* d_w, const HFr* x, size_t num_public, size_t room);
// d_e1 / d_e2 null: zero.  d_w_out (2^(l-1)) and d_e_out (2^l) may be input 1's.  Appends the proof (the T block)
std::vector<uint8_t> nova_fold(Ctx&, const Pcs&, const R1csKey&, const uint8_t* blob1, size_t len1, const uint8_t* blob2, size_t len2,
                               const Fr* d_w1, const Fr* d_e1, const Fr* d_w2, const Fr* d_e2, Fr* d_w_out, Fr* d_e_out, size_t room,
                               Transcript& tr);
std::vector<uint8_t> nova_fold_verify(size_t num_vars, size_t dim_vars, const uint8_t* key, size_t key_len, const uint8_t* blob1,
                                      size_t len1, const uint8_t* blob2, size_t len2, size_t room, Transcript& tr);
void spartan_prove_relaxed(Ctx&, const Pcs&, const R1csKey&, const uint8_t* blob, size_t len, const Fr* d_w, const Fr* d_e,
                           Transcript& tr);
void spartan_verify_relaxed(const PcsVerifier& pcs, size_t num_vars, size_t dim_vars, const uint8_t* key, size_t key_len,
                            const uint8_t* blob, size_t len, size_t num_public, Transcript& tr);
// the kernels alone (lh_debug_nova_spmv2, lh_debug_nova_cross_term)
void nova_debug_spmv2(Ctx&, const R1csKey&, int direction, const Fr* d_x1, const Fr* d_x2, Fr* const* d_out1, Fr* const* d_out2);

// ------------------------------------------------------------------ verifiers (verifier.cpp; host only)
HFr identity_eval(const std::vector<HFr>& x);  // sum_i 2^i x_i (sum_check.rs:123-125)
// verify_grand_product (oracle/pyref/gkr.py): trees of the given depths; -> the roots, and per tree the claim about its
// leaves' multilinear extension and the point it is made at.  A mismatch: LH_ERR_INVALID_SUMCHECK
struct GpClaim {
  HFr claim;
  std::vector<HFr> point;
};
std::vector<HFr> verify_grand_product(const std::vector<size_t>& depth, Transcript& tr, std::vector<GpClaim>& out);
HFr interpolate_evals(const std::vector<HFr>& evals, const HFr& x);  // barycentric over 0..d (arithmetic.rs:108-136)
HFr horner(const std::vector<HFr>& coeffs, const HFr& x);
struct VerifierParams;  // MultilinearKzgVerifierParams (kzg.rs:79-101)
VerifierParams* mkzg_vp_setup(const HFr* ss, size_t num_vars);
VerifierParams* mkzg_vp_new(const lh_g1& g1, const lh_g2& g2, const lh_g2* ss, size_t num_vars);
void mkzg_vp_export(const VerifierParams&, lh_g1* g1, lh_g2* g2, lh_g2* ss);
size_t mkzg_vp_num_vars(const VerifierParams&);
void mkzg_vp_free(VerifierParams*);
bool pairing_check(const lh_g1* ps, const lh_g2* qs, size_t n);
void mkzg_verify(const VerifierParams&, const HG1& comm, const HFr* point, size_t num_vars, const HFr& eval,
                 Transcript& tr);
void mkzg_batch_verify(const VerifierParams&, size_t num_vars, const HG1* comms, size_t num_comms, const HFr* points,
                       size_t num_points, const lh_evaluation* evals, size_t num_evals, Transcript& tr);
PcsVerifier mkzg_verifier(const VerifierParams&);
// -> (final claim, challenges)
std::pair<HFr, std::vector<HFr>> sum_check_verify(int prover_kind, size_t num_vars, size_t degree, const HFr& sum,
                                                  Transcript& tr);
// verify_fractional_sum_check (fractional_sum_check.rs:193-270; host only): claimed_*[b] null = the root is read.  The
// roots come back too: whoever argues with fractions checks a relation between them.  A mismatch: LH_ERR_INVALID_SUMCHECK
struct FracVerifyResult {
  std::vector<HFr> p_0s, q_0s, p_xs, q_xs, x;
};
FracVerifyResult verify_fractional_sum_check(size_t num_batching, size_t num_vars, const HFr* const* claimed_p_0s,
                                             const HFr* const* claimed_q_0s, Transcript& tr);
void lasso_verify(const PcsVerifier& pcs, const lh_lasso_table& table, size_t num_vars, Transcript& tr);
void lasso_verify_batch(const PcsVerifier& pcs, const lh_lasso_table* const* tables, size_t num_tables, size_t num_vars,
                        Transcript& tr);
// the verifier's side of lasso_argue: Surge and memory-checking identities; claims left to check against commitments
LassoClaims lasso_check(const lh_lasso_table& table, size_t num_vars, Transcript& tr);
void hyperplonk_verify(const PcsVerifier& pcs, const lh_hp_vparam& vp, const HFr* const* instances, Transcript& tr);
void hyperplonk_verify_phases(const PcsVerifier& pcs, const lh_hp_vparam& vp, const std::vector<size_t>& num_witness_polys,
                              const std::vector<size_t>& num_challenges, const HFr* const* instances, Transcript& tr);

// ------------------------------------------------------------------ HyperPlonk (hyperplonk.cpp)
void hyperplonk_prove(Ctx&, const Pcs&, const lh_hp_param& pp, const HFr* const* instances,
                      const Fr* const* d_witness, Transcript& tr);
// multi-phase circuits (hyperplonk.rs:185-205): phase r synthesizes num_witness_polys[r] device tables from the
// challenges of the earlier phases (PlonkishCircuit::synthesize, backend.rs:139), then num_challenges[r] are squeezed
struct HpPhases {
  std::vector<size_t> num_witness_polys, num_challenges;
  std::function<std::vector<const Fr*>(size_t round, const std::vector<HFr>& challenges)> synthesize;
};
HpPhases hp_single_phase(const lh_hp_param& pp, const Fr* const* d_witness);  // synthesize(0, []) = d_witness
void hyperplonk_prove_phases(Ctx&, const Pcs&, const lh_hp_param& pp, const HpPhases& phases,
                             const HFr* const* instances, Transcript& tr);

}  // namespace lh
