// extern "C" boundary: thin wrappers translating C++ exceptions into lh_status codes.
#include "host.hpp"
#include "brakedown.hpp"
#include <memory>

using namespace lh;

struct lh_ctx {
  Ctx c;
  explicit lh_ctx(int device_id) : c(device_id) {}
};
struct lh_srs {
  Srs s;
};
struct lh_mkzg_vp {
  VerifierParams* p;
};
struct lh_usrs {
  USrs s;
};
struct lh_zm_vp {
  ZmVerifierParams* p;
};
struct lh_ukzg_vp {
  UkzgVerifierParams* p;
};
struct lh_ipa_param {
  std::unique_ptr<IpaParams> p;
};
struct lh_brakedown_param {
  BdParam p;
};
struct lh_brakedown_comm {
  BdComm c;
};

#define LH_TRY try {
#define LH_CATCH                                  \
  }                                               \
  catch (const lh::Error& e) {                    \
    lh::set_last_error(e.what());                 \
    return e.code;                                \
  }                                               \
  catch (const std::exception& e) {               \
    lh::set_last_error(e.what());                 \
    return LH_ERR_DEVICE;                         \
  }                                               \
  return LH_OK;

#define NEED(p) LH_REQUIRE((p) != nullptr, LH_ERR_ARG, "null argument: " #p)
// (a vector argument may be null only when it is empty)
#define NEED_N(p, n) LH_REQUIRE((p) != nullptr || (n) == 0, LH_ERR_ARG, "null argument: " #p)

// The current HIP device is a per-host-thread setting: every entry point that takes a ctx makes the ctx's device
// current for the duration of the call (workspace growth, SRS shards and runtime-compiled modules must land on the
// device the ctx's stream belongs to, whichever thread calls) and restores the caller's device afterwards.
#define NEED_CTX(ctx) \
  NEED(ctx);          \
  OnDevice device_guard_((ctx)->c.device)

// ---------------------------------------------------------------- Lasso and HyperPlonk over any PCS: one body per kind of entry
// The exported functions (one per scheme, below) check their ctx and their own param handle and hand over the scheme's part
// as a callable that builds its Pcs / PcsVerifier.  It runs after the problem's pointers and the transcript are checked:
// which error a call with several defects reports is part of the boundary.  Hyrax's callables begin with its geometry check.

// the phase loop's arguments as the prover wants them (hyperplonk.rs:185-205); a single-phase circuit: hp_single_phase
static HpPhases hp_phases_of(const lh_hp_param* pp, size_t num_phases, const size_t* num_witness_polys,
                             const size_t* num_challenges, const lh_hp_circuit* circuit) {
  LH_REQUIRE(circuit->synthesize, LH_ERR_ARG, "circuit: synthesize callback missing");
  LH_REQUIRE(num_phases == 0 || (num_witness_polys && num_challenges), LH_ERR_ARG, "null argument: phases");
  HpPhases ph;
  ph.num_witness_polys.assign(num_witness_polys, num_witness_polys + num_phases);
  ph.num_challenges.assign(num_challenges, num_challenges + num_phases);
  size_t tw = 0, tc = 0;
  for (size_t r = 0; r < num_phases; r++) tw += num_witness_polys[r], tc += num_challenges[r];
  LH_REQUIRE(tw == pp->num_witness_polys && tc == pp->num_challenges, LH_ERR_ARG,
             "hyperplonk: phases do not add up to num_witness_polys / num_challenges");
  const std::vector<size_t> per_phase = ph.num_witness_polys;
  ph.synthesize = [circuit, per_phase](size_t round, const std::vector<HFr>& challenges) {
    std::vector<const void*> out(per_phase[round], nullptr);
    int rc = circuit->synthesize(circuit->user, round, (const lh_fr*)challenges.data(), challenges.size(), out.data(),
                                 out.size());
    if (rc != LH_OK) throw lh::Error(rc < 0 ? rc : LH_ERR_INVALID_SNARK, "circuit synthesize callback failed");
    std::vector<const Fr*> w;
    for (const void* p : out) {
      LH_REQUIRE(p != nullptr, LH_ERR_ARG, "circuit synthesize left a witness poly unset");
      w.push_back((const Fr*)p);
    }
    return w;
  };
  return ph;
}
// the per-phase counts as the verifier wants them
struct VerifierPhases {
  std::vector<size_t> num_witness_polys, num_challenges;
};
static VerifierPhases verifier_phases_of(size_t num_phases, const size_t* num_witness_polys, const size_t* num_challenges) {
  LH_REQUIRE(num_phases == 0 || (num_witness_polys && num_challenges), LH_ERR_ARG, "null argument: phases");
  return {std::vector<size_t>(num_witness_polys, num_witness_polys + num_phases),
          std::vector<size_t>(num_challenges, num_challenges + num_phases)};
}
// the communicator checks of the sharded entries; the proof is sharded while the returned object lives
static std::unique_ptr<ShardActive> shard_activate(Ctx& c, const char* entry) {
  LH_REQUIRE(c.has_comm, LH_ERR_ARG, std::string(entry) + ": no communicator attached");
  const size_t R = (size_t)c.comm.size;
  LH_REQUIRE(R >= 1 && (R & (R - 1)) == 0, LH_ERR_ARG, "sharded prove: the number of ranks must be a power of two");
  return std::unique_ptr<ShardActive>(new ShardActive(c));
}

template <class MakePcs>
static void lasso_prove_entry(Ctx& c, const lh_lasso_table* table, size_t num_vars, const uint32_t* const* d_dims,
                              lh_transcript* t, const MakePcs& make_pcs) {
  NEED(table);
  NEED(d_dims);
  Transcript tr(t);
  lasso_prove(c, make_pcs(), *table, num_vars, d_dims, tr);
}
template <class MakeVerifier>
static void lasso_verify_entry(const lh_lasso_table* table, size_t num_vars, lh_transcript* t, const MakeVerifier& make_verifier) {
  NEED(table);
  Transcript tr(t);
  lasso_verify(make_verifier(), *table, num_vars, tr);
}
template <class MakePcs>
static void hyperplonk_prove_entry(Ctx& c, const lh_hp_param* pp, const lh_fr* const* instances,
                                   const lh_fr* const* d_witness_polys, lh_transcript* t, const MakePcs& make_pcs) {
  NEED(pp);
  NEED_N(d_witness_polys, pp->num_witness_polys);
  Transcript tr(t);
  hyperplonk_prove(c, make_pcs(), *pp, (const HFr* const*)instances, (const Fr* const*)d_witness_polys, tr);
}
// `geometry` (Hyrax): its check of the circuit's size comes ahead of the phases' checks, its Pcs behind them
template <class MakePcs>
static void hyperplonk_prove_phases_entry(Ctx& c, const lh_hp_param* pp, size_t num_phases, const size_t* num_witness_polys,
                                          const size_t* num_challenges, const lh_fr* const* instances,
                                          const lh_hp_circuit* circuit, lh_transcript* t, const MakePcs& make_pcs,
                                          const std::function<void()>& geometry = nullptr) {
  NEED(pp);
  NEED(circuit);
  Transcript tr(t);
  if (geometry) geometry();
  const HpPhases ph = hp_phases_of(pp, num_phases, num_witness_polys, num_challenges, circuit);
  hyperplonk_prove_phases(c, make_pcs(), *pp, ph, (const HFr* const*)instances, tr);
}
template <class MakeVerifier>
static void hyperplonk_verify_entry(const lh_hp_vparam* hvp, const lh_fr* const* instances, lh_transcript* t,
                                    const MakeVerifier& make_verifier) {
  NEED(hvp);
  Transcript tr(t);
  hyperplonk_verify(make_verifier(), *hvp, (const HFr* const*)instances, tr);
}
template <class MakeVerifier>
static void hyperplonk_verify_phases_entry(const lh_hp_vparam* hvp, size_t num_phases, const size_t* num_witness_polys,
                                           const size_t* num_challenges, const lh_fr* const* instances, lh_transcript* t,
                                           const MakeVerifier& make_verifier) {
  NEED(hvp);
  const VerifierPhases ph = verifier_phases_of(num_phases, num_witness_polys, num_challenges);
  Transcript tr(t);
  hyperplonk_verify_phases(make_verifier(), *hvp, ph.num_witness_polys, ph.num_challenges, (const HFr* const*)instances, tr);
}
// Hyrax commits only tables of exactly the param's num_vars (hyrax.rs groups rows by the param's count): Lasso's tables ...
static void hyrax_lasso_vars(const IpaParams& p, size_t poly_size, size_t batch_size, const lh_lasso_table& tb, size_t num_vars) {
  const HyraxDims d = hyrax_trim(p, poly_size, batch_size);
  LH_REQUIRE(std::max<size_t>(num_vars, tb.chunk_bits) == d.num_vars, LH_ERR_ARG,
             "lasso over hyrax: max(num_vars, chunk_bits) must equal log2(poly_size) (Hyrax commits only tables of the param's size)");
}
// ... and the circuit's k
static void hyrax_hyperplonk_vars(const IpaParams& p, size_t poly_size, size_t batch_size, size_t num_vars) {
  const HyraxDims d = hyrax_trim(p, poly_size, batch_size);
  LH_REQUIRE(num_vars == d.num_vars, LH_ERR_ARG,
             "hyperplonk over hyrax: the circuit's num_vars must equal log2(poly_size) (Hyrax commits only tables of the param's size)");
}

extern "C" {

const char* lh_last_error(void) { return lh::get_last_error(); }
const char* lh_version(void) { return "lasso-hip 0.1 (gfx950)"; }

lh_status lh_ctx_create(int device_id, lh_ctx** out) {
  LH_TRY
  NEED(out);
  *out = new lh_ctx(device_id);  // (a constructor that throws has released what it made)
  LH_CATCH
}

void lh_ctx_destroy(lh_ctx* ctx) {
  if (!ctx) return;
  OnDevice on(ctx->c.device, true);
  delete ctx;
}

lh_status lh_ctx_sync(lh_ctx* ctx) {
  LH_TRY
  NEED_CTX(ctx);
  ctx->c.sync();
  LH_CATCH
}
void* lh_ctx_stream(lh_ctx* ctx) { return ctx ? (void*)ctx->c.stream : nullptr; }

lh_status lh_alloc(lh_ctx* ctx, size_t bytes, void** d_out) {
  LH_TRY
  NEED_CTX(ctx);
  NEED(d_out);
  LH_HIP(hipMalloc(d_out, bytes ? bytes : 1));
  LH_CATCH
}
lh_status lh_free(lh_ctx* ctx, void* d_ptr) {
  LH_TRY
  NEED_CTX(ctx);
  ctx->c.sync();
  if (d_ptr) LH_HIP(hipFree(d_ptr));
  LH_CATCH
}
lh_status lh_upload(lh_ctx* ctx, void* d_dst, const void* src, size_t bytes) {
  LH_TRY
  NEED_CTX(ctx);
  NEED_N(d_dst, bytes);
  NEED_N(src, bytes);
  if (bytes) {
    LH_HIP(hipMemcpyAsync(d_dst, src, bytes, hipMemcpyHostToDevice, ctx->c.stream));
    ctx->c.sync();
  }
  LH_CATCH
}
lh_status lh_download(lh_ctx* ctx, void* dst, const void* d_src, size_t bytes) {
  LH_TRY
  NEED_CTX(ctx);
  NEED_N(dst, bytes);
  NEED_N(d_src, bytes);
  if (bytes) {
    LH_HIP(hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, ctx->c.stream));
    ctx->c.sync();
  }
  LH_CATCH
}

// ---------------------------------------------------------------- transcript
lh_status lh_keccak_transcript_new(lh_transcript** out) {
  LH_TRY
  NEED(out);
  KeccakTranscript* t = new KeccakTranscript();
  *out = &t->vt;
  LH_CATCH
}
void lh_keccak_transcript_free(lh_transcript* t) {
  if (t) delete (KeccakTranscript*)t->user;
}
lh_status lh_keccak_transcript_proof(lh_transcript* t, const uint8_t** bytes, size_t* len) {
  LH_TRY
  NEED(t);
  NEED(bytes);
  NEED(len);
  KeccakTranscript* k = (KeccakTranscript*)t->user;
  *bytes = k->stream.data();
  *len = k->stream.size();
  LH_CATCH
}
lh_status lh_keccak_transcript_from_proof(const uint8_t* proof, size_t len, lh_transcript** out) {
  LH_TRY
  NEED(out);
  LH_REQUIRE(proof || !len, LH_ERR_ARG, "null argument: proof");
  KeccakTranscript* t = new KeccakTranscript();
  t->stream.assign(proof, proof + len);
  *out = &t->vt;
  LH_CATCH
}
lh_status lh_keccak_transcript_remaining(lh_transcript* t, size_t* out) {
  LH_TRY
  NEED(t);
  NEED(out);
  KeccakTranscript* k = (KeccakTranscript*)t->user;
  *out = k->stream.size() - k->pos;
  LH_CATCH
}

// ---------------------------------------------------------------- Fr vectors
lh_status lh_fr_from_u64(lh_ctx* ctx, const uint64_t* d_in, size_t n, lh_fr* d_out) {
  LH_TRY NEED_CTX(ctx);
  NEED_N(d_in, n);
  NEED_N(d_out, n);
  k_fr_from_u64(ctx->c, d_in, n, (Fr*)d_out);
  LH_CATCH
}
lh_status lh_fr_from_u32(lh_ctx* ctx, const uint32_t* d_in, size_t n, lh_fr* d_out) {
  LH_TRY NEED_CTX(ctx);
  NEED_N(d_in, n);
  NEED_N(d_out, n);
  k_fr_from_u32(ctx->c, d_in, n, (Fr*)d_out);
  LH_CATCH
}
lh_status lh_fr_to_repr(lh_ctx* ctx, const lh_fr* d_in, size_t n, uint8_t* d_out32) {
  LH_TRY NEED_CTX(ctx);
  NEED_N(d_in, n);
  NEED_N(d_out32, n);
  k_fr_to_repr(ctx->c, (const Fr*)d_in, n, (Fr*)d_out32);
  LH_CATCH
}
lh_status lh_fr_from_repr(lh_ctx* ctx, const uint8_t* d_in32, size_t n, lh_fr* d_out) {
  LH_TRY NEED_CTX(ctx);
  NEED_N(d_in32, n);
  NEED_N(d_out, n);
  k_fr_from_repr(ctx->c, (const Fr*)d_in32, n, (Fr*)d_out);
  LH_CATCH
}
lh_status lh_fr_add(lh_ctx* ctx, const lh_fr* a, const lh_fr* b, size_t n, lh_fr* out) {
  LH_TRY NEED_CTX(ctx);
  NEED_N(a, n);
  NEED_N(b, n);
  NEED_N(out, n);
  k_fr_binop(ctx->c, 0, (const Fr*)a, (const Fr*)b, n, (Fr*)out);
  LH_CATCH
}
lh_status lh_fr_sub(lh_ctx* ctx, const lh_fr* a, const lh_fr* b, size_t n, lh_fr* out) {
  LH_TRY NEED_CTX(ctx);
  NEED_N(a, n);
  NEED_N(b, n);
  NEED_N(out, n);
  k_fr_binop(ctx->c, 1, (const Fr*)a, (const Fr*)b, n, (Fr*)out);
  LH_CATCH
}
lh_status lh_fr_mul(lh_ctx* ctx, const lh_fr* a, const lh_fr* b, size_t n, lh_fr* out) {
  LH_TRY NEED_CTX(ctx);
  NEED_N(a, n);
  NEED_N(b, n);
  NEED_N(out, n);
  k_fr_binop(ctx->c, 2, (const Fr*)a, (const Fr*)b, n, (Fr*)out);
  LH_CATCH
}
lh_status lh_fr_mul_chain(lh_ctx* ctx, const lh_fr* a, const lh_fr* b, size_t n, int iters, lh_fr* out) {
  LH_TRY NEED_CTX(ctx);
  NEED_N(a, n);
  NEED_N(b, n);
  NEED_N(out, n);
  k_fr_mul_chain(ctx->c, (const Fr*)a, (const Fr*)b, n, iters, (Fr*)out);
  LH_CATCH
}
lh_status lh_fr_batch_invert(lh_ctx* ctx, const lh_fr* d_in, size_t n, lh_fr* d_out) {
  LH_TRY NEED_CTX(ctx);
  NEED_N(d_in, n);
  NEED_N(d_out, n);
  k_fr_batch_invert(ctx->c, (const Fr*)d_in, n, (Fr*)d_out);
  LH_CATCH
}

// ---------------------------------------------------------------- MultilinearPolynomial
static bool is_pow2(size_t n) { return n && !(n & (n - 1)); }

lh_status lh_fix_var(lh_ctx* ctx, const lh_fr* d_in, size_t n_in, const lh_fr* x, lh_fr* d_out) {
  LH_TRY NEED_CTX(ctx);
  NEED(x);
  NEED(d_in);
  NEED(d_out);
  LH_REQUIRE(is_pow2(n_in) && n_in >= 2, LH_ERR_ARG, "fix_var: table must have 2^m >= 2 entries");
  Fr xr;
  memcpy(&xr, x, 32);
  k_fix_var(ctx->c, (const Fr*)d_in, n_in, xr, (Fr*)d_out);
  LH_CATCH
}
lh_status lh_eq_xy(lh_ctx* ctx, const lh_fr* y, size_t num_vars, lh_fr* d_out) {
  LH_TRY NEED_CTX(ctx);
  NEED_N(y, num_vars);
  NEED(d_out);
  LH_REQUIRE(num_vars < 32, LH_ERR_ARG, "eq_xy: num_vars too large");
  k_eq_xy(ctx->c, (const Fr*)y, num_vars, (Fr*)d_out);
  LH_CATCH
}
lh_status lh_evaluate(lh_ctx* ctx, const lh_fr* const* d_polys, size_t num_polys, size_t num_vars,
                      const lh_fr* point, lh_fr* out_evals) {
  LH_TRY NEED_CTX(ctx);
  NEED_N(d_polys, num_polys);
  NEED_N(out_evals, num_polys);
  NEED_N(point, num_vars);
  std::vector<HFr> ev = evaluate_polys(ctx->c, (const Fr* const*)d_polys, num_polys, num_vars, (const HFr*)point);
  memcpy(out_evals, ev.data(), num_polys * 32);
  LH_CATCH
}
lh_status lh_lincomb(lh_ctx* ctx, const lh_fr* const* d_polys, const lh_fr* w, size_t num_polys, size_t n,
                     lh_fr* d_out) {
  LH_TRY NEED_CTX(ctx);
  NEED_N(d_polys, num_polys);
  NEED_N(w, num_polys);
  NEED_N(d_out, n);
  k_lincomb(ctx->c, (const Fr* const*)d_polys, (const Fr*)w, num_polys, n, (Fr*)d_out);
  LH_CATCH
}

// ---------------------------------------------------------------- sum-check / GKR
lh_status lh_sumcheck_prove(lh_ctx* ctx, int prover_kind, size_t num_vars, const lh_sop* expr,
                            const lh_fr* const* d_polys, size_t num_polys, const lh_fr* ys, size_t num_ys,
                            const lh_fr* sum, lh_transcript* t, lh_fr* out_challenges, lh_fr* out_evals) {
  LH_TRY NEED_CTX(ctx);
  NEED(expr);
  NEED(sum);
  NEED_N(d_polys, num_polys);
  NEED_N(ys, num_ys);
  LH_REQUIRE(prover_kind == LH_SC_EVALUATIONS || prover_kind == LH_SC_COEFFICIENTS, LH_ERR_ARG, "bad prover kind");
  Transcript tr(t);
  HFr s;
  memcpy(&s, sum, 32);
  SumCheckResult r = sum_check_prove(ctx->c, prover_kind, num_vars, *expr, (const Fr* const*)d_polys, num_polys,
                                     (const HFr*)ys, num_ys, s, tr);
  if (out_challenges) memcpy(out_challenges, r.challenges.data(), r.challenges.size() * 32);
  if (out_evals) memcpy(out_evals, r.evals.data(), r.evals.size() * 32);
  LH_CATCH
}

lh_status lh_sumcheck_prove_expr(lh_ctx* ctx, size_t num_vars, const lh_expr* expr, const lh_fr* const* d_polys,
                                 size_t num_polys, const lh_fr* challenges, size_t num_challenges, const lh_fr* ys,
                                 size_t num_ys, const lh_fr* sum, lh_transcript* t, lh_fr* out_challenges,
                                 lh_fr* out_evals) {
  LH_TRY NEED_CTX(ctx);
  NEED(expr);
  NEED(sum);
  NEED_N(d_polys, num_polys);
  NEED_N(challenges, num_challenges);
  NEED_N(ys, num_ys);
  Transcript tr(t);
  HFr s;
  memcpy(&s, sum, 32);
  SumCheckResult r = sum_check_prove_expr(ctx->c, num_vars, *expr, (const Fr* const*)d_polys, num_polys,
                                          (const HFr*)challenges, num_challenges, (const HFr*)ys, num_ys, s, tr);
  if (out_challenges) memcpy(out_challenges, r.challenges.data(), r.challenges.size() * 32);
  if (out_evals) memcpy(out_evals, r.evals.data(), r.evals.size() * 32);
  LH_CATCH
}

lh_status lh_gkr_fractional_prove(lh_ctx* ctx, size_t num_batching, size_t num_vars,
                                  const lh_fr* const* claimed_p_0s, const lh_fr* const* claimed_q_0s,
                                  const lh_fr* const* d_ps, const lh_fr* const* d_qs, lh_transcript* t,
                                  lh_fr* out_p_xs, lh_fr* out_q_xs, lh_fr* out_x) {
  LH_TRY NEED_CTX(ctx);
  NEED_N(claimed_p_0s, num_batching);
  NEED_N(claimed_q_0s, num_batching);
  NEED_N(d_ps, num_batching);
  NEED_N(d_qs, num_batching);
  Transcript tr(t);
  FracSumCheckResult r =
      prove_fractional_sum_check(ctx->c, num_batching, num_vars, (const HFr* const*)claimed_p_0s,
                                 (const HFr* const*)claimed_q_0s, (const Fr* const*)d_ps, (const Fr* const*)d_qs, tr);
  if (out_p_xs) memcpy(out_p_xs, r.p_xs.data(), r.p_xs.size() * 32);
  if (out_q_xs) memcpy(out_q_xs, r.q_xs.data(), r.q_xs.size() * 32);
  if (out_x) memcpy(out_x, r.x.data(), r.x.size() * 32);
  LH_CATCH
}

lh_status lh_grand_product_prove(lh_ctx* ctx, size_t num_trees, const lh_fr* const* d_leaves, const size_t* num_vars,
                                 lh_transcript* t, lh_fr* out_roots, lh_fr* out_claims, lh_fr* out_points) {
  LH_TRY NEED_CTX(ctx);
  NEED(num_vars);
  NEED_N(d_leaves, num_trees);
  Transcript tr(t);
  GrandProductResult r = prove_grand_product(ctx->c, num_trees, (const Fr* const*)d_leaves, num_vars, tr);
  if (out_roots) memcpy(out_roots, r.roots.data(), num_trees * 32);
  if (out_claims) memcpy(out_claims, r.claims.data(), num_trees * 32);
  if (out_points) {
    lh_fr* p = out_points;
    for (size_t b = 0; b < num_trees; b++) {
      memcpy(p, r.points[b].data(), r.points[b].size() * 32);
      p += r.points[b].size();
    }
  }
  LH_CATCH
}

// ---------------------------------------------------------------- MSM
lh_status lh_msm(lh_ctx* ctx, const lh_fr* d_scalars, const lh_g1* d_bases, size_t n, lh_g1* out) {
  LH_TRY NEED_CTX(ctx);
  NEED(out);
  NEED_N(d_scalars, n);
  NEED_N(d_bases, n);
  MsmJob job{d_scalars, false, (const G1Affine*)d_bases, n};
  msm_batch(ctx->c, &job, 1, (G1Affine*)out);
  LH_CATCH
}
lh_status lh_msm_u32(lh_ctx* ctx, const uint32_t* d_scalars, const lh_g1* d_bases, size_t n, lh_g1* out) {
  LH_TRY NEED_CTX(ctx);
  NEED(out);
  NEED_N(d_scalars, n);
  NEED_N(d_bases, n);
  MsmJob job{d_scalars, true, (const G1Affine*)d_bases, n};
  msm_batch(ctx->c, &job, 1, (G1Affine*)out);
  LH_CATCH
}

// ---------------------------------------------------------------- multilinear KZG
lh_status lh_mkzg_setup(lh_ctx* ctx, const lh_fr* ss, size_t num_vars, lh_srs** out) {
  LH_TRY NEED_CTX(ctx);
  NEED(out);
  NEED_N(ss, num_vars);
  *out = new lh_srs{mkzg_setup(ctx->c, (const HFr*)ss, num_vars)};
  LH_CATCH
}
lh_status lh_srs_upload(lh_ctx* ctx, const lh_g1* eqs_flat, size_t num_vars, lh_srs** out) {
  LH_TRY NEED_CTX(ctx);
  NEED(out);
  NEED(eqs_flat);
  LH_REQUIRE(num_vars < 31, LH_ERR_ARG, "srs: num_vars too large");
  std::unique_ptr<lh_srs> w(new lh_srs());
  w->s.num_vars = num_vars;
  size_t total = ((size_t)2 << num_vars) - 1;
  w->s.d_eqs.alloc(total * sizeof(G1Affine));
  if (hipMemcpyAsync(w->s.d_eqs, eqs_flat, total * sizeof(G1Affine), hipMemcpyHostToDevice, ctx->c.stream) != hipSuccess ||
      hipStreamSynchronize(ctx->c.stream) != hipSuccess)
    throw lh::Error(LH_ERR_DEVICE, "srs upload failed");
  *out = w.release();
  LH_CATCH
}
lh_status lh_srs_download(lh_ctx* ctx, const lh_srs* srs, lh_g1* eqs_flat) {
  LH_TRY NEED_CTX(ctx);
  NEED(srs);
  NEED(eqs_flat);
  size_t total = ((size_t)2 << srs->s.num_vars) - 1;
  LH_HIP(hipMemcpyAsync(eqs_flat, srs->s.d_eqs, total * sizeof(G1Affine), hipMemcpyDeviceToHost, ctx->c.stream));
  ctx->c.sync();
  LH_CATCH
}
size_t lh_srs_num_vars(const lh_srs* srs) { return srs ? srs->s.num_vars : 0; }
void lh_srs_free(lh_ctx* ctx, lh_srs* srs) {
  if (!srs) return;
  if (ctx) (void)hipStreamSynchronize(ctx->c.stream);
  delete srs;
}

lh_status lh_mkzg_commit(lh_ctx* ctx, const lh_srs* srs, const lh_fr* d_poly, size_t num_vars, lh_g1* out) {
  LH_TRY NEED_CTX(ctx);
  NEED(srs);
  NEED(d_poly);
  NEED(out);
  const Fr* p = (const Fr*)d_poly;
  std::vector<HG1> c = mkzg_batch_commit(ctx->c, srs->s, &p, 1, num_vars);
  memcpy(out, c.data(), 64);
  LH_CATCH
}
lh_status lh_mkzg_batch_commit(lh_ctx* ctx, const lh_srs* srs, const lh_fr* const* d_polys, size_t num_polys,
                               size_t num_vars, lh_g1* out_comms) {
  LH_TRY NEED_CTX(ctx);
  NEED(srs);
  NEED_N(d_polys, num_polys);
  NEED_N(out_comms, num_polys);
  std::vector<HG1> c = mkzg_batch_commit(ctx->c, srs->s, (const Fr* const*)d_polys, num_polys, num_vars);
  if (num_polys) memcpy(out_comms, c.data(), num_polys * 64);
  LH_CATCH
}
lh_status lh_mkzg_open(lh_ctx* ctx, const lh_srs* srs, const lh_fr* d_poly, size_t num_vars, const lh_fr* point,
                       lh_transcript* t, lh_fr* out_eval) {
  LH_TRY NEED_CTX(ctx);
  NEED(srs);
  NEED(d_poly);
  NEED_N(point, num_vars);
  Transcript tr(t);
  HFr e = mkzg_open(ctx->c, srs->s, (const Fr*)d_poly, num_vars, (const HFr*)point, tr);
  if (out_eval) memcpy(out_eval, &e, 32);
  LH_CATCH
}
lh_status lh_mkzg_batch_open(lh_ctx* ctx, const lh_srs* srs, size_t num_vars, const lh_fr* const* d_polys,
                             size_t num_polys, const lh_fr* points, size_t num_points, const lh_evaluation* evals,
                             size_t num_evals, lh_transcript* t) {
  LH_TRY NEED_CTX(ctx);
  NEED(srs);
  NEED_N(d_polys, num_polys);
  NEED_N(points, num_points);
  NEED_N(evals, num_evals);
  Transcript tr(t);
  mkzg_batch_open(ctx->c, srs->s, num_vars, (const Fr* const*)d_polys, num_polys, (const HFr*)points, num_points,
                  evals, num_evals, tr);
  LH_CATCH
}

// ---------------------------------------------------------------- Lasso
lh_status lh_lasso_prove(lh_ctx* ctx, const lh_srs* srs, const lh_lasso_table* table, size_t num_vars,
                         const uint32_t* const* d_dims, lh_transcript* t) {
  LH_TRY NEED_CTX(ctx);
  NEED(srs);
  lasso_prove_entry(ctx->c, table, num_vars, d_dims, t, [&] { return mkzg_pcs(ctx->c, srs->s); });
  LH_CATCH
}
lh_status lh_lasso_prove_batch(lh_ctx* ctx, const lh_srs* srs, const lh_lasso_table* const* tables, size_t num_tables,
                               size_t num_vars, const uint32_t* const* const* d_dims, lh_transcript* t) {
  LH_TRY NEED_CTX(ctx);
  NEED(srs);
  NEED(tables);
  NEED(d_dims);
  Transcript tr(t);
  lasso_prove_batch(ctx->c, mkzg_pcs(ctx->c, srs->s), tables, num_tables, num_vars, d_dims, tr);
  LH_CATCH
}
// ---------------------------------------------------------------- LogUp-GKR
lh_status lh_logup_gkr_prove(lh_ctx* ctx, const lh_srs* srs, const lh_logup_lookup* lookups, size_t num_lookups, size_t num_vars,
                             size_t table_vars, lh_transcript* t) {
  LH_TRY NEED_CTX(ctx);
  NEED(srs);
  NEED(lookups);
  Transcript tr(t);
  logup_gkr_prove(ctx->c, mkzg_pcs(ctx->c, srs->s), lookups, num_lookups, num_vars, table_vars, tr);
  LH_CATCH
}
lh_status lh_logup_gkr_prove_columns(lh_ctx* ctx, const lh_srs* srs, const lh_logup_columns* lookups, size_t num_lookups,
                                     size_t num_vars, size_t table_vars, lh_transcript* t) {
  LH_TRY NEED_CTX(ctx);
  NEED(srs);
  NEED(lookups);
  Transcript tr(t);
  logup_gkr_prove_columns(ctx->c, mkzg_pcs(ctx->c, srs->s), lookups, num_lookups, num_vars, table_vars, tr);
  LH_CATCH
}
// ---------------------------------------------------------------- read-write memory checking
lh_status lh_memcheck_prove(lh_ctx* ctx, const lh_srs* srs, const lh_memcheck_trace* trace, size_t num_vars, size_t mem_vars,
                            const uint32_t* init, lh_transcript* t) {
  LH_TRY NEED_CTX(ctx);
  NEED(srs);
  NEED(trace);
  Transcript tr(t);
  memcheck_prove(ctx->c, mkzg_pcs(ctx->c, srs->s), *trace, num_vars, mem_vars, init, tr);
  LH_CATCH
}
lh_status lh_memcheck_replay(lh_ctx* ctx, const lh_memcheck_ops* ops, size_t num_vars, size_t mem_vars, const uint32_t* d_image,
                             uint32_t* d_rv, uint32_t* d_wv, uint32_t* d_final) {
  LH_TRY
  memcheck_check(num_vars, mem_vars, false);  // (the shape first: refused before the device is touched)
  NEED_CTX(ctx);
  NEED(ops);
  NEED(d_rv);
  NEED(d_wv);
  memcheck_replay(ctx->c, *ops, num_vars, mem_vars, d_image, d_rv, d_wv, d_final);
  LH_CATCH
}
lh_status lh_memcheck_prove_segment(lh_ctx* ctx, const lh_srs* srs, const lh_memcheck_trace* trace, size_t num_vars, size_t mem_vars,
                                    const uint32_t* d_image, uint32_t* d_final, lh_transcript* t) {
  LH_TRY
  memcheck_segment_check(num_vars, mem_vars);
  NEED_CTX(ctx);
  NEED(srs);
  NEED(trace);
  NEED(d_image);
  Transcript tr(t);
  memcheck_prove_segment(ctx->c, mkzg_pcs(ctx->c, srs->s), *trace, num_vars, mem_vars, d_image, d_final, tr);
  LH_CATCH
}
// ---------------------------------------------------------------- Spark: commit a sparse polynomial once, open it many times
lh_status lh_spark_commit(lh_ctx* ctx, const lh_srs* srs, size_t num_vars, size_t dim_vars, size_t num_dims,
                          const uint32_t* const* d_dims, const lh_fr* d_val, lh_spark_poly** out) {
  LH_TRY
  spark_check(num_vars, dim_vars, num_dims);  // (the shape first: refused before the param or the device is touched)
  NEED_CTX(ctx);
  NEED(srs);
  NEED(out);
  *out = nullptr;
  *out = (lh_spark_poly*)spark_commit(ctx->c, mkzg_pcs(ctx->c, srs->s), num_vars, dim_vars, num_dims, d_dims, (const Fr*)d_val);
  LH_CATCH
}
lh_status lh_spark_commitment(const lh_spark_poly* poly, uint8_t* out, size_t* len) {
  LH_TRY
  NEED(poly);
  NEED(len);
  const std::vector<uint8_t>& blob = ((const SparkPoly*)poly)->blob;
  if (out) {
    LH_REQUIRE(*len >= blob.size(), LH_ERR_ARG, "spark: the buffer is shorter than the commitment");
    memcpy(out, blob.data(), blob.size());
  }
  *len = blob.size();
  LH_CATCH
}
lh_status lh_spark_open(lh_ctx* ctx, const lh_srs* srs, const lh_spark_poly* poly, const lh_fr* point, lh_fr* out_value,
                        lh_transcript* t) {
  LH_TRY NEED_CTX(ctx);
  NEED(srs);
  NEED(poly);
  NEED(point);
  NEED(out_value);
  Transcript tr(t);
  const HFr v = spark_open(ctx->c, mkzg_pcs(ctx->c, srs->s), *(const SparkPoly*)poly, (const HFr*)point, tr);
  memcpy(out_value, &v, 32);
  LH_CATCH
}
void lh_spark_free(lh_ctx* ctx, lh_spark_poly* poly) {
  if (!ctx || !poly) return;
  spark_free(ctx->c, (SparkPoly*)poly);
}
// ---------------------------------------------------------------- Spartan: R1CS over the Spark-committed matrices
lh_status lh_r1cs_commit(lh_ctx* ctx, const lh_srs* srs, size_t num_vars, size_t dim_vars, const lh_r1cs_matrix m[3],
                         lh_r1cs_key** out) {
  LH_TRY
  spartan_check(num_vars, dim_vars, 1);  // (the shape first: refused before the param or the device is touched)
  NEED_CTX(ctx);
  NEED(srs);
  NEED(m);
  NEED(out);
  *out = nullptr;
  *out = (lh_r1cs_key*)spartan_commit(ctx->c, mkzg_pcs(ctx->c, srs->s), num_vars, dim_vars, m);
  LH_CATCH
}
lh_status lh_r1cs_commitment(const lh_r1cs_key* key, uint8_t* out, size_t* len) {
  LH_TRY
  NEED(key);
  NEED(len);
  const std::vector<uint8_t>& blob = ((const R1csKey*)key)->blob;
  if (out) {
    LH_REQUIRE(*len >= blob.size(), LH_ERR_ARG, "spartan: the buffer is shorter than the key");
    memcpy(out, blob.data(), blob.size());
  }
  *len = blob.size();
  LH_CATCH
}
lh_status lh_spartan_prove(lh_ctx* ctx, const lh_srs* srs, const lh_r1cs_key* key, const lh_fr* d_w, const lh_fr* x,
                           size_t num_public, lh_transcript* t) {
  LH_TRY NEED_CTX(ctx);
  NEED(srs);
  NEED(key);
  NEED(d_w);
  NEED(x);
  Transcript tr(t);
  spartan_prove(ctx->c, mkzg_pcs(ctx->c, srs->s), *(const R1csKey*)key, (const Fr*)d_w, (const HFr*)x, num_public, tr);
  LH_CATCH
}
void lh_r1cs_free(lh_ctx* ctx, lh_r1cs_key* key) {
  if (!ctx || !key) return;
  spartan_free(ctx->c, (R1csKey*)key);
}
// ---------------------------------------------------------------- Nova folding over an R1CS key; relaxed Spartan
// an entry's instance blob goes to the caller's buffer: *len is the room in - the entry checks it against
// LH_NOVA_INSTANCE_BYTES(num_public) before any work - and the length out
static size_t nova_blob_room(const uint8_t* out, const size_t* len) {
  LH_REQUIRE(out != nullptr && len != nullptr, LH_ERR_ARG, "null argument: out_instance or out_len");
  return *len;
}
static void nova_blob_out(const std::vector<uint8_t>& blob, uint8_t* out, size_t* len) {
  memcpy(out, blob.data(), blob.size());
  *len = blob.size();
}
lh_status lh_nova_instance(lh_ctx* ctx, const lh_srs* srs, const lh_r1cs_key* key, const lh_fr* d_w, const lh_fr* x, size_t num_public,
                           uint8_t* out_instance, size_t* out_len) {
  LH_TRY NEED_CTX(ctx);
  NEED(srs);
  NEED(key);
  NEED(d_w);
  NEED(x);
  const size_t room = nova_blob_room(out_instance, out_len);
  nova_blob_out(nova_instance(ctx->c, mkzg_pcs(ctx->c, srs->s), *(const R1csKey*)key, (const Fr*)d_w, (const HFr*)x, num_public, room),
                out_instance, out_len);
  LH_CATCH
}
lh_status lh_nova_fold(lh_ctx* ctx, const lh_srs* srs, const lh_r1cs_key* key, const uint8_t* instance1, size_t instance1_len,
                       const uint8_t* instance2, size_t instance2_len, const lh_fr* d_w1, const lh_fr* d_e1, const lh_fr* d_w2,
                       const lh_fr* d_e2, lh_fr* d_w_out, lh_fr* d_e_out, uint8_t* out_instance, size_t* out_len, lh_transcript* t) {
  LH_TRY NEED_CTX(ctx);
  NEED(srs);
  NEED(key);
  NEED(instance1);
  NEED(instance2);
  NEED(d_w1);
  NEED(d_w2);
  NEED(d_w_out);
  NEED(d_e_out);
  Transcript tr(t);
  const size_t room = nova_blob_room(out_instance, out_len);
  nova_blob_out(nova_fold(ctx->c, mkzg_pcs(ctx->c, srs->s), *(const R1csKey*)key, instance1, instance1_len, instance2, instance2_len,
                          (const Fr*)d_w1, (const Fr*)d_e1, (const Fr*)d_w2, (const Fr*)d_e2, (Fr*)d_w_out, (Fr*)d_e_out, room, tr),
                out_instance, out_len);
  LH_CATCH
}
lh_status lh_spartan_prove_relaxed(lh_ctx* ctx, const lh_srs* srs, const lh_r1cs_key* key, const uint8_t* instance, size_t instance_len,
                                   const lh_fr* d_w, const lh_fr* d_e, lh_transcript* t) {
  LH_TRY NEED_CTX(ctx);
  NEED(srs);
  NEED(key);
  NEED(instance);
  NEED(d_w);
  Transcript tr(t);
  spartan_prove_relaxed(ctx->c, mkzg_pcs(ctx->c, srs->s), *(const R1csKey*)key, instance, instance_len, (const Fr*)d_w, (const Fr*)d_e, tr);
  LH_CATCH
}
lh_status lh_lasso_last_timing(lh_ctx* ctx, double* out_ms) {
  LH_TRY NEED_CTX(ctx);
  NEED(out_ms);
  ctx->c.phase_times_resolve();  // (the phase boundaries are events on the stream: lasso.cpp lap)
  memcpy(out_ms, ctx->c.lasso_ms, sizeof(ctx->c.lasso_ms));
  LH_CATCH
}

lh_status lh_ctx_set_option(lh_ctx* ctx, const char* name, int64_t value) {
  LH_TRY NEED_CTX(ctx);
  int64_t* slot = ctx->c.opt.find(name);
  LH_REQUIRE(slot != nullptr, LH_ERR_ARG, std::string("unknown option: ") + (name ? name : "(null)"));
  LH_REQUIRE(Options::in_range(name, value), LH_ERR_ARG, std::string("option value out of range: ") + name);
  *slot = value;
  if (slot == &ctx->c.opt.open_small_min_vars) ctx->c.opt.open_small_min_vars_forced = true;
  LH_CATCH
}
lh_status lh_ctx_get_option(lh_ctx* ctx, const char* name, int64_t* out) {
  LH_TRY NEED_CTX(ctx);
  NEED(out);
  int64_t* slot = ctx->c.opt.find(name);
  LH_REQUIRE(slot != nullptr, LH_ERR_ARG, std::string("unknown option: ") + (name ? name : "(null)"));
  *out = *slot;
  LH_CATCH
}
lh_status lh_lasso_last_route(lh_ctx* ctx, lh_lasso_route* out) {
  LH_TRY NEED_CTX(ctx);
  NEED(out);
  static_assert(sizeof(lh_lasso_route) == sizeof(uint32_t) * LH_LASSO_ROUTE_WORDS, "lh_lasso_route layout");
  memcpy(out, ctx->c.route.v, sizeof(*out));
  LH_CATCH
}

// caller-registered subtables (subtable.cpp): host only, no ctx
lh_status lh_subtable_register(const uint32_t* values, uint32_t chunk_bits, uint32_t* out_kind) {
  LH_TRY
  NEED(values);
  NEED(out_kind);
  *out_kind = subtable_register(values, chunk_bits);
  LH_CATCH
}
lh_status lh_subtable_unregister(uint32_t kind) {
  LH_TRY
  subtable_unregister(kind);
  LH_CATCH
}
lh_status lh_subtable_info(uint32_t kind, uint32_t* chunk_bits, uint32_t* value_bits, uint8_t digest32[32]) {
  LH_TRY
  const std::shared_ptr<const CustomSubtable> t = subtable_find(kind);
  LH_REQUIRE(t != nullptr, LH_ERR_ARG, "subtable: not a registered kind");
  if (chunk_bits) *chunk_bits = t->chunk_bits;
  if (value_bits) *value_bits = t->value_bits;
  if (digest32) memcpy(digest32, t->digest, 32);
  LH_CATCH
}

lh_status lh_ctx_set_comm(lh_ctx* ctx, const lh_comm* comm, size_t shard_bit) {
  LH_TRY NEED_CTX(ctx);
  ctx->c.sync();
  comm_detach(ctx->c);
  if (comm) {
    LH_REQUIRE(comm->size >= 1 && (comm->size & (comm->size - 1)) == 0 && comm->rank >= 0 && comm->rank < comm->size,
               LH_ERR_ARG, "communicator: size must be a power of two and 0 <= rank < size");
    LH_REQUIRE(comm->all_gather || comm->all_gather_device, LH_ERR_ARG, "communicator: no all_gather callback");
    ctx->c.comm = *comm;
    ctx->c.has_comm = true;
    ctx->c.shard_bit = shard_bit;
    ctx->c.comm_stats[0] = ctx->c.comm_stats[1] = 0;
  }
  LH_CATCH
}
lh_status lh_rccl_unique_id(uint8_t out[LH_RCCL_UNIQUE_ID_BYTES]) {
  LH_TRY
  NEED(out);
  rccl_unique_id(out);
  LH_CATCH
}
lh_status lh_ctx_set_comm_rccl(lh_ctx* ctx, int rank, int size, const uint8_t unique_id[LH_RCCL_UNIQUE_ID_BYTES],
                               size_t shard_bit) {
  LH_TRY NEED_CTX(ctx);
  NEED(unique_id);
  LH_REQUIRE(size >= 1 && (size & (size - 1)) == 0 && rank >= 0 && rank < size, LH_ERR_ARG,
             "communicator: size must be a power of two and 0 <= rank < size");
  ctx->c.sync();
  comm_attach_rccl(ctx->c, rank, size, unique_id, shard_bit);
  ctx->c.comm_stats[0] = ctx->c.comm_stats[1] = 0;
  LH_CATCH
}
lh_status lh_ctx_set_comm_loopback(lh_ctx* ctx, int rank, int size, size_t shard_bit) {
  LH_TRY NEED_CTX(ctx);
  LH_REQUIRE(size >= 1 && (size & (size - 1)) == 0 && rank >= 0 && rank < size, LH_ERR_ARG,
             "communicator: size must be a power of two and 0 <= rank < size");
  ctx->c.sync();
  comm_attach_loopback(ctx->c, rank, size, shard_bit);
  ctx->c.comm_stats[0] = ctx->c.comm_stats[1] = 0;
  LH_CATCH
}
lh_status lh_ctx_comm_stats(lh_ctx* ctx, uint64_t out[2]) {
  LH_TRY NEED_CTX(ctx);
  NEED(out);
  out[0] = ctx->c.comm_stats[0];
  out[1] = ctx->c.comm_stats[1];
  LH_CATCH
}
lh_status lh_ctx_comm_phase_stats(lh_ctx* ctx, uint64_t out[16], int reset) {
  LH_TRY NEED_CTX(ctx);
  NEED(out);
  for (int p = 0; p < 8; p++) {
    out[2 * p] = ctx->c.comm_phase_stats[p][0];
    out[2 * p + 1] = ctx->c.comm_phase_stats[p][1];
    if (reset) ctx->c.comm_phase_stats[p][0] = ctx->c.comm_phase_stats[p][1] = 0;
  }
  LH_CATCH
}
lh_status lh_ctx_memory_stats(lh_ctx* ctx, uint64_t out[4]) {
  LH_TRY NEED_CTX(ctx);
  NEED(out);
  out[0] = ctx->c.arena.high_water() + (ctx->c.helper ? ctx->c.helper->arena.high_water() : 0);
  out[1] = ctx->c.arena.reserved() + (ctx->c.helper ? ctx->c.helper->arena.reserved() : 0);
  size_t free_b = 0, total_b = 0;
  LH_HIP(hipMemGetInfo(&free_b, &total_b));
  out[2] = free_b, out[3] = total_b;
  LH_CATCH
}
lh_status lh_ctx_compute_units(lh_ctx* ctx, size_t* out) {
  LH_TRY NEED_CTX(ctx);
  NEED(out);
  *out = (size_t)ctx->c.num_cus;
  LH_CATCH
}
lh_status lh_ctx_host_cpus(lh_ctx* ctx, char* bus_id, size_t bus_id_cap, char* cpulist, size_t cpulist_cap) {
  LH_TRY NEED_CTX(ctx);
  NEED(bus_id);
  NEED(cpulist);
  LH_REQUIRE(bus_id_cap >= 16 && cpulist_cap >= 2, LH_ERR_ARG, "host cpus: buffers too small");
  char id[64] = {0};
  LH_HIP(hipDeviceGetPCIBusId(id, (int)sizeof(id), ctx->c.device));
  for (char* p = id; *p; p++) *p = (char)tolower((unsigned char)*p);  // (sysfs spells the address in lower case)
  snprintf(bus_id, bus_id_cap, "%s", id);
  cpulist[0] = 0;
  const std::string path = std::string("/sys/bus/pci/devices/") + id + "/local_cpulist";
  if (FILE* f = fopen(path.c_str(), "r")) {
    if (fgets(cpulist, (int)cpulist_cap, f)) {
      size_t n = strlen(cpulist);
      while (n && (cpulist[n - 1] == '\n' || cpulist[n - 1] == ' ')) cpulist[--n] = 0;
    } else {
      cpulist[0] = 0;
    }
    fclose(f);
  }
  LH_CATCH
}
// ONE proof over the 2^rho ranks of the ctx's communicator: the same prover, with every table a shard
// (dev.hpp Shard).  Same transcript, same proof bytes on every rank as lasso_prove on one GPU.
lh_status lh_lasso_prove_sharded(lh_ctx* ctx, const lh_srs* srs, const lh_lasso_table* table, size_t num_vars,
                                 const uint32_t* const* d_dims, lh_transcript* t) {
  LH_TRY NEED_CTX(ctx);
  NEED(srs);
  std::unique_ptr<ShardActive> active;
  lasso_prove_entry(ctx->c, table, num_vars, d_dims, t, [&] {
    active = shard_activate(ctx->c, "lasso_prove_sharded");
    return mkzg_pcs(ctx->c, srs->s);
  });
  LH_CATCH
}

lh_status lh_hyperplonk_prove_phases(lh_ctx* ctx, const lh_srs* srs, const lh_hp_param* pp, size_t num_phases,
                                     const size_t* num_witness_polys, const size_t* num_challenges,
                                     const lh_fr* const* instances, const lh_hp_circuit* circuit, lh_transcript* t) {
  LH_TRY NEED_CTX(ctx);
  NEED(srs);
  hyperplonk_prove_phases_entry(ctx->c, pp, num_phases, num_witness_polys, num_challenges, instances, circuit, t,
                                [&] { return mkzg_pcs(ctx->c, srs->s); });
  LH_CATCH
}

lh_status lh_hyperplonk_prove(lh_ctx* ctx, const lh_srs* srs, const lh_hp_param* pp, const lh_fr* const* instances,
                              const lh_fr* const* d_witness_polys, lh_transcript* t) {
  LH_TRY NEED_CTX(ctx);
  NEED(srs);
  hyperplonk_prove_entry(ctx->c, pp, instances, d_witness_polys, t, [&] { return mkzg_pcs(ctx->c, srs->s); });
  LH_CATCH
}

lh_status lh_shard_extract(lh_ctx* ctx, const void* d_global, size_t n_local, size_t shard_bit, size_t rho, size_t rank,
                           size_t elem_bytes, void* d_local) {
  LH_TRY NEED_CTX(ctx);
  NEED(d_global);
  NEED(d_local);
  LH_REQUIRE(rho < 16 && rank < ((size_t)1 << rho) && shard_bit < 40, LH_ERR_ARG, "shard_extract: bad geometry");
  k_shard_extract(ctx->c, d_global, n_local, shard_bit, rho, rank, elem_bytes, d_local);
  ctx->c.sync();
  LH_CATCH
}
lh_status lh_hyperplonk_prove_sharded(lh_ctx* ctx, const lh_srs* srs, const lh_hp_param* pp, const lh_fr* const* instances,
                                      const lh_fr* const* d_witness_polys, lh_transcript* t) {
  LH_TRY NEED_CTX(ctx);
  NEED(srs);
  NEED(pp);  // (the communicator is checked behind the circuit's pointers and ahead of the transcript)
  NEED_N(d_witness_polys, pp->num_witness_polys);
  const std::unique_ptr<ShardActive> active = shard_activate(ctx->c, "lh_hyperplonk_prove_sharded");
  hyperplonk_prove_entry(ctx->c, pp, instances, d_witness_polys, t, [&] { return mkzg_pcs(ctx->c, srs->s); });
  LH_CATCH
}

// ---------------------------------------------------------------- verifiers (host only)
lh_status lh_mkzg_vp_setup(const lh_fr* ss, size_t num_vars, lh_mkzg_vp** out) {
  LH_TRY
  NEED(out);
  LH_REQUIRE(ss || !num_vars, LH_ERR_ARG, "null argument: ss");
  *out = new lh_mkzg_vp{mkzg_vp_setup((const HFr*)ss, num_vars)};
  LH_CATCH
}
lh_status lh_mkzg_vp_new(const lh_g1* g1, const lh_g2* g2, const lh_g2* ss, size_t num_vars, lh_mkzg_vp** out) {
  LH_TRY
  NEED(out);
  NEED(g1);
  NEED(g2);
  LH_REQUIRE(ss || !num_vars, LH_ERR_ARG, "null argument: ss");
  *out = new lh_mkzg_vp{mkzg_vp_new(*g1, *g2, ss, num_vars)};
  LH_CATCH
}
lh_status lh_mkzg_vp_export(const lh_mkzg_vp* vp, lh_g1* g1, lh_g2* g2, lh_g2* ss) {
  LH_TRY
  NEED(vp);
  NEED(g1);
  NEED(g2);
  NEED_N(ss, mkzg_vp_num_vars(*vp->p));
  mkzg_vp_export(*vp->p, g1, g2, ss);
  LH_CATCH
}
size_t lh_mkzg_vp_num_vars(const lh_mkzg_vp* vp) { return vp ? mkzg_vp_num_vars(*vp->p) : 0; }
void lh_mkzg_vp_free(lh_mkzg_vp* vp) {
  if (!vp) return;
  mkzg_vp_free(vp->p);
  delete vp;
}
lh_status lh_pairing_check(const lh_g1* ps, const lh_g2* qs, size_t n, int* out_is_identity) {
  LH_TRY
  NEED(out_is_identity);
  LH_REQUIRE((ps && qs) || !n, LH_ERR_ARG, "null argument: points");
  *out_is_identity = pairing_check(ps, qs, n) ? 1 : 0;
  LH_CATCH
}
lh_status lh_mkzg_verify(const lh_mkzg_vp* vp, const lh_g1* comm, const lh_fr* point, size_t num_vars,
                         const lh_fr* eval, lh_transcript* t) {
  LH_TRY
  NEED(vp);
  NEED(comm);
  NEED(eval);
  LH_REQUIRE(point || !num_vars, LH_ERR_ARG, "null argument: point");
  Transcript tr(t);
  HG1 c;
  memcpy(&c, comm, sizeof(c));
  HFr e;
  memcpy(&e, eval, 32);
  mkzg_verify(*vp->p, c, (const HFr*)point, num_vars, e, tr);
  LH_CATCH
}
lh_status lh_mkzg_batch_verify(const lh_mkzg_vp* vp, size_t num_vars, const lh_g1* comms, size_t num_comms,
                               const lh_fr* points, size_t num_points, const lh_evaluation* evals, size_t num_evals,
                               lh_transcript* t) {
  LH_TRY
  NEED(vp);
  NEED_N(comms, num_comms);
  NEED_N(points, num_points);
  NEED_N(evals, num_evals);
  Transcript tr(t);
  mkzg_batch_verify(*vp->p, num_vars, (const HG1*)comms, num_comms, (const HFr*)points, num_points, evals, num_evals,
                    tr);
  LH_CATCH
}
lh_status lh_sumcheck_verify(int prover_kind, size_t num_vars, size_t degree, const lh_fr* sum, lh_transcript* t,
                             lh_fr* out_eval, lh_fr* out_x) {
  LH_TRY
  NEED(sum);
  Transcript tr(t);
  HFr s;
  memcpy(&s, sum, 32);
  auto res = sum_check_verify(prover_kind, num_vars, degree, s, tr);
  if (out_eval) memcpy(out_eval, &res.first, 32);
  if (out_x) memcpy(out_x, res.second.data(), 32 * res.second.size());
  LH_CATCH
}
lh_status lh_lasso_verify(const lh_mkzg_vp* vp, const lh_lasso_table* table, size_t num_vars, lh_transcript* t) {
  LH_TRY
  NEED(vp);
  lasso_verify_entry(table, num_vars, t, [&] { return mkzg_verifier(*vp->p); });
  LH_CATCH
}
lh_status lh_lasso_verify_batch(const lh_mkzg_vp* vp, const lh_lasso_table* const* tables, size_t num_tables, size_t num_vars,
                                lh_transcript* t) {
  LH_TRY
  NEED(vp);
  NEED(tables);
  Transcript tr(t);
  if (lasso_batch_check(tables, num_tables, num_vars) > mkzg_vp_num_vars(*vp->p))
    throw lh::Error(LH_ERR_INVALID_PCS_PARAM, "Too many variates of poly to verify");
  lasso_verify_batch(mkzg_verifier(*vp->p), tables, num_tables, num_vars, tr);
  LH_CATCH
}
lh_status lh_gkr_fractional_verify(size_t num_batching, size_t num_vars, const lh_fr* const* claimed_p_0s,
                                   const lh_fr* const* claimed_q_0s, lh_transcript* t, lh_fr* out_p_0s, lh_fr* out_q_0s,
                                   lh_fr* out_p_xs, lh_fr* out_q_xs, lh_fr* out_x) {
  LH_TRY
  Transcript tr(t);
  const FracVerifyResult r = verify_fractional_sum_check(num_batching, num_vars, (const HFr* const*)claimed_p_0s,
                                                         (const HFr* const*)claimed_q_0s, tr);
  if (out_p_0s) memcpy(out_p_0s, r.p_0s.data(), r.p_0s.size() * 32);
  if (out_q_0s) memcpy(out_q_0s, r.q_0s.data(), r.q_0s.size() * 32);
  if (out_p_xs) memcpy(out_p_xs, r.p_xs.data(), r.p_xs.size() * 32);
  if (out_q_xs) memcpy(out_q_xs, r.q_xs.data(), r.q_xs.size() * 32);
  if (out_x) memcpy(out_x, r.x.data(), r.x.size() * 32);
  LH_CATCH
}
lh_status lh_logup_gkr_verify(const lh_mkzg_vp* vp, const lh_logup_lookup* lookups, size_t num_lookups, size_t num_vars,
                              size_t table_vars, lh_transcript* t) {
  LH_TRY
  NEED(vp);
  NEED(lookups);
  Transcript tr(t);
  if (logup_check(lookups, num_lookups, num_vars, table_vars, false) > mkzg_vp_num_vars(*vp->p))
    throw lh::Error(LH_ERR_INVALID_PCS_PARAM, "Too many variates of poly to verify");
  logup_gkr_verify(mkzg_verifier(*vp->p), lookups, num_lookups, num_vars, table_vars, tr);
  LH_CATCH
}
lh_status lh_memcheck_verify(const lh_mkzg_vp* vp, size_t num_vars, size_t mem_vars, const uint32_t* init, lh_transcript* t) {
  LH_TRY
  NEED(vp);
  Transcript tr(t);
  if (memcheck_check(num_vars, mem_vars, init != nullptr) > mkzg_vp_num_vars(*vp->p))
    throw lh::Error(LH_ERR_INVALID_PCS_PARAM, "Too many variates of poly to verify");
  memcheck_verify(mkzg_verifier(*vp->p), num_vars, mem_vars, init, tr);
  LH_CATCH
}
lh_status lh_memcheck_verify_segment(const lh_mkzg_vp* vp, size_t num_vars, size_t mem_vars, lh_transcript* t,
                                     lh_g1* image_commitment, lh_g1* final_commitment) {
  LH_TRY
  NEED(vp);
  Transcript tr(t);
  if (memcheck_segment_check(num_vars, mem_vars) > mkzg_vp_num_vars(*vp->p))
    throw lh::Error(LH_ERR_INVALID_PCS_PARAM, "Too many variates of poly to verify");
  HG1 iv, fv;
  memcheck_verify_segment(mkzg_verifier(*vp->p), num_vars, mem_vars, tr, &iv, &fv);
  if (image_commitment) memcpy(image_commitment, &iv, 64);
  if (final_commitment) memcpy(final_commitment, &fv, 64);
  LH_CATCH
}
lh_status lh_spark_verify(const lh_mkzg_vp* vp, size_t num_vars, size_t dim_vars, size_t num_dims, const uint8_t* commitment,
                          size_t commitment_len, const lh_fr* point, const lh_fr* value, lh_transcript* t) {
  LH_TRY
  NEED(vp);
  NEED(commitment);
  NEED(point);
  NEED(value);
  Transcript tr(t);
  if (spark_check(num_vars, dim_vars, num_dims) > mkzg_vp_num_vars(*vp->p))
    throw lh::Error(LH_ERR_INVALID_PCS_PARAM, "Too many variates of poly to verify");
  HFr v;
  memcpy(&v, value, 32);
  spark_verify(mkzg_verifier(*vp->p), num_vars, dim_vars, num_dims, commitment, commitment_len, (const HFr*)point, v, tr);
  LH_CATCH
}
lh_status lh_spartan_verify(const lh_mkzg_vp* vp, size_t num_vars, size_t dim_vars, const uint8_t* commitment, size_t commitment_len,
                            const lh_fr* x, size_t num_public, lh_transcript* t) {
  LH_TRY
  NEED(vp);
  NEED(commitment);
  NEED(x);
  Transcript tr(t);
  if (spartan_check(num_vars, dim_vars, num_public) > mkzg_vp_num_vars(*vp->p))
    throw lh::Error(LH_ERR_INVALID_PCS_PARAM, "Too many variates of poly to verify");
  spartan_verify(mkzg_verifier(*vp->p), num_vars, dim_vars, commitment, commitment_len, (const HFr*)x, num_public, tr);
  LH_CATCH
}
lh_status lh_nova_fold_verify(size_t num_vars, size_t dim_vars, const uint8_t* commitment, size_t commitment_len, const uint8_t* instance1,
                              size_t instance1_len, const uint8_t* instance2, size_t instance2_len, uint8_t* out_instance, size_t* out_len,
                              lh_transcript* t) {
  LH_TRY
  spartan_check(num_vars, dim_vars, 1);
  NEED(commitment);
  NEED(instance1);
  NEED(instance2);
  Transcript tr(t);
  const size_t room = nova_blob_room(out_instance, out_len);
  nova_blob_out(nova_fold_verify(num_vars, dim_vars, commitment, commitment_len, instance1, instance1_len, instance2, instance2_len, room,
                                 tr),
                out_instance, out_len);
  LH_CATCH
}
lh_status lh_spartan_verify_relaxed(const lh_mkzg_vp* vp, size_t num_vars, size_t dim_vars, const uint8_t* commitment, size_t commitment_len,
                                    const uint8_t* instance, size_t instance_len, size_t num_public, lh_transcript* t) {
  LH_TRY
  NEED(vp);
  NEED(commitment);
  NEED(instance);
  Transcript tr(t);
  if (spartan_check(num_vars, dim_vars, num_public) > mkzg_vp_num_vars(*vp->p))
    throw lh::Error(LH_ERR_INVALID_PCS_PARAM, "Too many variates of poly to verify");
  spartan_verify_relaxed(mkzg_verifier(*vp->p), num_vars, dim_vars, commitment, commitment_len, instance, instance_len, num_public, tr);
  LH_CATCH
}
lh_status lh_spartan_verify_batch(const lh_mkzg_vp* vp, size_t num_vars, size_t dim_vars, const uint8_t* commitment, size_t commitment_len,
                                  const lh_fr* x, size_t num_instances, size_t num_public, lh_transcript* t) {
  LH_TRY
  NEED(vp);
  NEED(commitment);
  NEED(x);
  Transcript tr(t);
  spartan_check(num_vars, dim_vars, num_public);
  if (std::max(num_vars, spartan_batch_check(dim_vars, num_instances) + dim_vars - 1) > mkzg_vp_num_vars(*vp->p))
    throw lh::Error(LH_ERR_INVALID_PCS_PARAM, "Too many variates of poly to verify");
  spartan_verify_batch(mkzg_verifier(*vp->p), num_vars, dim_vars, commitment, commitment_len, (const HFr*)x, num_instances, num_public, tr);
  LH_CATCH
}
lh_status lh_hyperplonk_verify(const lh_mkzg_vp* vp, const lh_hp_vparam* hvp, const lh_fr* const* instances,
                               lh_transcript* t) {
  LH_TRY
  NEED(vp);
  hyperplonk_verify_entry(hvp, instances, t, [&] { return mkzg_verifier(*vp->p); });
  LH_CATCH
}
lh_status lh_hyperplonk_verify_phases(const lh_mkzg_vp* vp, const lh_hp_vparam* hvp, size_t num_phases,
                                      const size_t* num_witness_polys, const size_t* num_challenges,
                                      const lh_fr* const* instances, lh_transcript* t) {
  LH_TRY
  NEED(vp);
  hyperplonk_verify_phases_entry(hvp, num_phases, num_witness_polys, num_challenges, instances, t,
                                 [&] { return mkzg_verifier(*vp->p); });
  LH_CATCH
}

// ---------------------------------------------------------------- Zeromorph over univariate KZG
lh_status lh_ukzg_setup(lh_ctx* ctx, const lh_fr* s, size_t poly_size, lh_usrs** out) {
  LH_TRY NEED_CTX(ctx);
  NEED(s);
  NEED(out);
  HFr sv;
  memcpy(&sv, s, 32);
  *out = new lh_usrs{ukzg_setup(ctx->c, sv, poly_size)};
  LH_CATCH
}
lh_status lh_usrs_upload(lh_ctx* ctx, const lh_g1* powers, size_t poly_size, lh_usrs** out) {
  LH_TRY NEED_CTX(ctx);
  NEED(powers);
  NEED(out);
  LH_REQUIRE(poly_size >= 1 && poly_size < ((size_t)1 << 31), LH_ERR_ARG, "univariate srs: bad poly_size");
  std::unique_ptr<lh_usrs> w(new lh_usrs());
  w->s.size = poly_size;
  w->s.d_powers.alloc(poly_size * sizeof(G1Affine));
  if (hipMemcpyAsync(w->s.d_powers, powers, poly_size * sizeof(G1Affine), hipMemcpyHostToDevice, ctx->c.stream) != hipSuccess ||
      hipStreamSynchronize(ctx->c.stream) != hipSuccess)
    throw lh::Error(LH_ERR_DEVICE, "univariate srs upload failed");
  *out = w.release();
  LH_CATCH
}
lh_status lh_usrs_download(lh_ctx* ctx, const lh_usrs* srs, lh_g1* powers) {
  LH_TRY NEED_CTX(ctx);
  NEED(srs);
  NEED(powers);
  LH_HIP(hipMemcpyAsync(powers, srs->s.d_powers, srs->s.size * sizeof(G1Affine), hipMemcpyDeviceToHost, ctx->c.stream));
  ctx->c.sync();
  LH_CATCH
}
size_t lh_usrs_size(const lh_usrs* srs) { return srs ? srs->s.size : 0; }
void lh_usrs_free(lh_ctx* ctx, lh_usrs* srs) {
  if (!srs) return;
  if (ctx) (void)hipStreamSynchronize(ctx->c.stream);
  delete srs;
}
lh_status lh_zeromorph_batch_commit(lh_ctx* ctx, const lh_usrs* srs, size_t poly_size, const lh_fr* const* d_polys,
                                    size_t num_polys, size_t num_vars, lh_g1* out_comms) {
  LH_TRY NEED_CTX(ctx);
  NEED(srs);
  LH_REQUIRE((d_polys && out_comms) || !num_polys, LH_ERR_ARG, "null argument: polys");
  std::vector<HG1> c = zeromorph_batch_commit(ctx->c, srs->s, poly_size, (const Fr* const*)d_polys, num_polys, num_vars);
  if (num_polys) memcpy(out_comms, c.data(), 64 * num_polys);
  LH_CATCH
}
lh_status lh_zeromorph_open(lh_ctx* ctx, const lh_usrs* srs, size_t poly_size, const lh_fr* d_poly, size_t num_vars,
                            const lh_fr* point, lh_transcript* t) {
  LH_TRY NEED_CTX(ctx);
  NEED(srs);
  NEED(d_poly);
  NEED_N(point, num_vars);
  Transcript tr(t);
  zeromorph_open(ctx->c, srs->s, poly_size, (const Fr*)d_poly, num_vars, (const HFr*)point, tr);
  LH_CATCH
}
lh_status lh_zeromorph_batch_open(lh_ctx* ctx, const lh_usrs* srs, size_t poly_size, size_t num_vars,
                                  const lh_fr* const* d_polys, size_t num_polys, const lh_fr* points,
                                  size_t num_points, const lh_evaluation* evals, size_t num_evals, lh_transcript* t) {
  LH_TRY NEED_CTX(ctx);
  NEED(srs);
  NEED_N(d_polys, num_polys);
  NEED_N(points, num_points);
  NEED_N(evals, num_evals);
  Transcript tr(t);
  zeromorph_batch_open(ctx->c, srs->s, poly_size, num_vars, (const Fr* const*)d_polys, num_polys, (const HFr*)points,
                       num_points, evals, num_evals, tr);
  LH_CATCH
}
lh_status lh_zeromorph_vp_setup(const lh_fr* s, size_t param_size, size_t poly_size, lh_zm_vp** out) {
  LH_TRY
  NEED(s);
  NEED(out);
  HFr sv;
  memcpy(&sv, s, 32);
  *out = new lh_zm_vp{zeromorph_vp_setup(sv, param_size, poly_size)};
  LH_CATCH
}
lh_status lh_zeromorph_vp_new(const lh_g1* g1, const lh_g2* g2, const lh_g2* s_g2, const lh_g2* s_offset_g2,
                              lh_zm_vp** out) {
  LH_TRY
  NEED(g1);
  NEED(g2);
  NEED(s_g2);
  NEED(s_offset_g2);
  NEED(out);
  *out = new lh_zm_vp{zeromorph_vp_new(*g1, *g2, *s_g2, *s_offset_g2)};
  LH_CATCH
}
lh_status lh_zeromorph_vp_export(const lh_zm_vp* vp, lh_g1* g1, lh_g2* g2, lh_g2* s_g2, lh_g2* s_offset_g2) {
  LH_TRY
  NEED(vp);
  NEED(g1);
  NEED(g2);
  NEED(s_g2);
  NEED(s_offset_g2);
  zeromorph_vp_export(*vp->p, g1, g2, s_g2, s_offset_g2);
  LH_CATCH
}
void lh_zeromorph_vp_free(lh_zm_vp* vp) {
  if (!vp) return;
  zeromorph_vp_free(vp->p);
  delete vp;
}
lh_status lh_zeromorph_verify(const lh_zm_vp* vp, const lh_g1* comm, const lh_fr* point, size_t num_vars,
                              const lh_fr* eval, lh_transcript* t) {
  LH_TRY
  NEED(vp);
  NEED(comm);
  NEED(eval);
  LH_REQUIRE(point || !num_vars, LH_ERR_ARG, "null argument: point");
  Transcript tr(t);
  HG1 c;
  memcpy(&c, comm, sizeof(c));
  HFr e;
  memcpy(&e, eval, 32);
  zeromorph_verify(*vp->p, c, (const HFr*)point, num_vars, e, tr);
  LH_CATCH
}
lh_status lh_zeromorph_batch_verify(const lh_zm_vp* vp, size_t num_vars, const lh_g1* comms, size_t num_comms,
                                    const lh_fr* points, size_t num_points, const lh_evaluation* evals,
                                    size_t num_evals, lh_transcript* t) {
  LH_TRY
  NEED(vp);
  NEED_N(comms, num_comms);
  NEED_N(points, num_points);
  NEED_N(evals, num_evals);
  Transcript tr(t);
  zeromorph_batch_verify(*vp->p, num_vars, (const HG1*)comms, num_comms, (const HFr*)points, num_points, evals,
                         num_evals, tr);
  LH_CATCH
}

// ---------------------------------------------------------------- Brakedown
lh_status lh_keccak_transcript_hash_io(lh_transcript* t, lh_hash_transcript* out) {
  LH_TRY
  NEED(t);
  NEED(out);
  LH_REQUIRE(keccak_transcript_hash_io(t, out), LH_ERR_ARG, "not the built-in Keccak256 transcript");
  LH_CATCH
}
lh_status lh_brakedown_setup(lh_ctx* ctx, size_t num_vars, int spec, const uint8_t* seed32, lh_brakedown_param** out) {
  LH_TRY
  NEED(seed32);
  NEED(out);
  OnDevice on(ctx ? ctx->c.device : -1);
  *out = new lh_brakedown_param{brakedown_setup(ctx ? &ctx->c : nullptr, num_vars, spec, seed32)};
  LH_CATCH
}
lh_status lh_brakedown_derive(size_t num_vars, int spec, lh_brakedown_param** out) {
  LH_TRY
  NEED(out);
  std::unique_ptr<lh_brakedown_param> w(new lh_brakedown_param());
  brakedown_derive(w->p, num_vars, spec);
  *out = w.release();
  LH_CATCH
}
lh_status lh_ligero_setup(lh_ctx* ctx, size_t num_vars, int log_inv_rate, size_t row_vars, lh_brakedown_param** out) {
  LH_TRY
  NEED(out);
  OnDevice on(ctx ? ctx->c.device : -1);
  *out = new lh_brakedown_param{ligero_setup(ctx ? &ctx->c : nullptr, num_vars, log_inv_rate, row_vars)};
  LH_CATCH
}
lh_status lh_ligero_derive(size_t num_vars, int log_inv_rate, size_t row_vars, lh_brakedown_param** out) {
  LH_TRY
  NEED(out);
  std::unique_ptr<lh_brakedown_param> w(new lh_brakedown_param());
  ligero_derive(w->p, num_vars, log_inv_rate, row_vars);
  *out = w.release();
  LH_CATCH
}
lh_status lh_brakedown_param_info(const lh_brakedown_param* pp, size_t* row_len, size_t* num_rows, size_t* codeword_len,
                                  size_t* num_column_opening, size_t* num_proximity_testing) {
  LH_TRY
  NEED(pp);
  NEED(row_len);
  NEED(num_rows);
  NEED(codeword_len);
  NEED(num_column_opening);
  NEED(num_proximity_testing);
  *row_len = pp->p.row_len, *num_rows = pp->p.num_rows, *codeword_len = pp->p.codeword_len;
  *num_column_opening = pp->p.num_column_opening, *num_proximity_testing = pp->p.num_proximity_testing;
  LH_CATCH
}
lh_status lh_brakedown_trim(const lh_brakedown_param* pp, size_t poly_size) {
  LH_TRY
  NEED(pp);
  brakedown_trim(pp->p, poly_size);
  LH_CATCH
}
void lh_brakedown_param_free(lh_brakedown_param* pp) { delete pp; }
lh_status lh_brakedown_encode(const lh_brakedown_param* pp, const lh_fr* msg, lh_fr* out) {
  LH_TRY
  NEED(pp);
  NEED(msg);
  NEED(out);
  std::vector<HFr> cw(pp->p.codeword_len);
  memcpy(cw.data(), msg, pp->p.row_len * 32);
  brakedown_encode_host(pp->p, cw.data());
  memcpy(out, cw.data(), cw.size() * 32);
  LH_CATCH
}
// `as_batch`: the polys as one batch of launches (brakedown.cpp brakedown_batch_commit); lh_brakedown_commit keeps its own
// kernels and launch shape
static lh_status bd_commit_entry(lh_ctx* ctx, const lh_brakedown_param* pp, const lh_fr* const* d_polys, size_t num_polys,
                                 size_t num_vars, lh_brakedown_comm** out, bool as_batch) {
  LH_TRY NEED_CTX(ctx);
  NEED(pp);
  NEED_N(d_polys, num_polys);
  NEED_N(out, num_polys);
  for (size_t i = 0; i < num_polys; i++) LH_REQUIRE(d_polys[i], LH_ERR_ARG, "null argument: d_polys[i]");
  std::vector<std::unique_ptr<lh_brakedown_comm>> comms;
  // batch_commit is one commit per poly (brakedown.rs:198-210): as one batch of launches, or literally
  std::vector<std::unique_ptr<BdComm>> batch;
  if (as_batch && num_polys && ctx->c.opt.brakedown_batch_commit)
    batch = brakedown_batch_commit(ctx->c, pp->p, (const Fr* const*)d_polys, num_polys, num_vars);
  for (size_t i = 0; i < num_polys; i++) {
    std::unique_ptr<BdComm> c = batch.empty() ? brakedown_commit(ctx->c, pp->p, (const Fr*)d_polys[i], num_vars) : std::move(batch[i]);
    comms.emplace_back(new lh_brakedown_comm{std::move(*c)});
  }
  for (size_t i = 0; i < num_polys; i++) out[i] = comms[i].release();
  LH_CATCH
}
lh_status lh_brakedown_commit(lh_ctx* ctx, const lh_brakedown_param* pp, const lh_fr* d_poly, size_t num_vars,
                              lh_brakedown_comm** out) {
  return bd_commit_entry(ctx, pp, d_poly ? &d_poly : nullptr, 1, num_vars, out, false);
}
lh_status lh_brakedown_batch_commit(lh_ctx* ctx, const lh_brakedown_param* pp, const lh_fr* const* d_polys,
                                    size_t num_polys, size_t num_vars, lh_brakedown_comm** out) {
  return bd_commit_entry(ctx, pp, d_polys, num_polys, num_vars, out, true);
}
lh_status lh_brakedown_commit_columns(lh_ctx* ctx, const lh_brakedown_param* pp, const void* const* d_cols, const int* kinds,
                                      const size_t* lens, size_t num_cols, lh_brakedown_comm** out) {
  LH_TRY NEED_CTX(ctx);
  NEED(pp);
  NEED_N(d_cols, num_cols);
  NEED_N(kinds, num_cols);
  NEED_N(lens, num_cols);
  NEED_N(out, num_cols);
  std::vector<BdColumn> cols(num_cols);
  for (size_t i = 0; i < num_cols; i++) {
    LH_REQUIRE(kinds[i] == LH_BD_COLUMN_FR || kinds[i] == LH_BD_COLUMN_U32, LH_ERR_ARG, "brakedown commit_columns: unknown kind");
    LH_REQUIRE(d_cols[i] || !lens[i], LH_ERR_ARG, "null argument: d_cols[i]");
    cols[i] = BdColumn{d_cols[i], lens[i], kinds[i] == LH_BD_COLUMN_U32 ? 1u : 0u, 0};
  }
  std::vector<std::unique_ptr<BdComm>> batch = brakedown_commit_columns(ctx->c, pp->p, cols.data(), num_cols);
  std::vector<std::unique_ptr<lh_brakedown_comm>> comms;
  for (size_t i = 0; i < num_cols; i++) {
    comms.emplace_back(new lh_brakedown_comm{std::move(*batch[i])});
  }
  for (size_t i = 0; i < num_cols; i++) out[i] = comms[i].release();
  LH_CATCH
}
lh_status lh_brakedown_comm_root(const lh_brakedown_comm* comm, uint8_t* out32) {
  LH_TRY
  NEED(comm);
  NEED(out32);
  memcpy(out32, comm->c.root, 32);
  LH_CATCH
}
lh_status lh_brakedown_comm_rows(lh_ctx* ctx, const lh_brakedown_comm* comm, lh_fr* out) {
  LH_TRY NEED_CTX(ctx);
  NEED(comm);
  NEED(out);
  LH_HIP(hipMemcpyAsync(out, comm->c.d_rows, comm->c.num_rows * comm->c.codeword_len * 32, hipMemcpyDeviceToHost,
                        ctx->c.stream));
  ctx->c.sync();
  LH_CATCH
}
lh_status lh_brakedown_comm_rows_device(const lh_brakedown_comm* comm, lh_fr** d_out) {
  LH_TRY
  NEED(comm);
  NEED(d_out);
  *d_out = (lh_fr*)comm->c.d_rows;
  LH_CATCH
}
lh_status lh_brakedown_comm_tree(lh_ctx* ctx, const lh_brakedown_comm* comm, uint8_t* out) {
  LH_TRY NEED_CTX(ctx);
  NEED(comm);
  NEED(out);
  LH_HIP(hipMemcpyAsync(out, comm->c.d_hashes, (((size_t)2 << comm->c.depth) - 1) * 32, hipMemcpyDeviceToHost,
                        ctx->c.stream));
  ctx->c.sync();
  LH_CATCH
}
lh_status lh_brakedown_comm_stage(lh_ctx* ctx, const lh_brakedown_param* pp, const lh_brakedown_comm* comm, lh_fr* out) {
  LH_TRY NEED_CTX(ctx);
  NEED(pp);
  NEED(comm);
  NEED(out);
  BdStage st;
  brakedown_stage(ctx->c, pp->p, comm->c, st);
  memcpy(out, st.cols, comm->c.num_rows * comm->c.codeword_len * 32);
  LH_CATCH
}
void lh_brakedown_comm_free(lh_brakedown_comm* comm) { delete comm; }
lh_status lh_brakedown_open(lh_ctx* ctx, const lh_brakedown_param* pp, const lh_fr* d_poly, size_t num_vars,
                            lh_brakedown_comm* comm, const lh_fr* point, lh_transcript* t, lh_hash_transcript* ht) {
  LH_TRY NEED_CTX(ctx);
  NEED(pp);
  NEED(d_poly);
  NEED(comm);
  NEED_N(point, num_vars);
  Transcript tr(t);
  HashTranscript h(ht);
  brakedown_open(ctx->c, pp->p, (const Fr*)d_poly, num_vars, comm->c, (const HFr*)point, tr, h);
  LH_CATCH
}
lh_status lh_brakedown_batch_open(lh_ctx* ctx, const lh_brakedown_param* pp, size_t num_vars, const lh_fr* const* d_polys,
                                  lh_brakedown_comm* const* comms, size_t num_polys, const lh_fr* points,
                                  size_t num_points, const lh_evaluation* evals, size_t num_evals, lh_transcript* t,
                                  lh_hash_transcript* ht) {
  LH_TRY NEED_CTX(ctx);
  NEED(pp);
  NEED_N(d_polys, num_polys);
  NEED_N(comms, num_polys);
  NEED_N(points, num_points);
  NEED_N(evals, num_evals);
  Transcript tr(t);
  HashTranscript h(ht);
  BdStage stage;  // (option brakedown_staged_open; freed with this call)
  const bool staged = ctx->c.opt.brakedown_staged_open != 0;
  for (size_t i = 0; i < num_evals; i++) {  // one open per evaluation (brakedown.rs:278-300)
    const lh_evaluation& e = evals[i];
    LH_REQUIRE(e.poly < num_polys && e.point < num_points && d_polys[e.poly] && comms[e.poly], LH_ERR_ARG,
               "brakedown batch_open: evaluation out of range");
    if (staged) brakedown_stage(ctx->c, pp->p, comms[e.poly]->c, stage);
    brakedown_open(ctx->c, pp->p, (const Fr*)d_polys[e.poly], num_vars, comms[e.poly]->c,
                   (const HFr*)points + (size_t)e.point * num_vars, tr, h, staged ? &stage : nullptr);
  }
  LH_CATCH
}
lh_status lh_brakedown_read_commitments(const lh_brakedown_param* pp, size_t num, lh_hash_transcript* ht, uint8_t* out) {
  LH_TRY
  NEED(pp);
  NEED_N(out, num);
  HashTranscript h(ht);
  for (size_t i = 0; i < num; i++) h.read_hash(out + 32 * i);
  LH_CATCH
}
lh_status lh_brakedown_verify(const lh_brakedown_param* pp, const uint8_t* root32, const lh_fr* point, size_t num_vars,
                              const lh_fr* eval, lh_transcript* t, lh_hash_transcript* ht) {
  LH_TRY
  NEED(pp);
  NEED(root32);
  NEED(eval);
  NEED_N(point, num_vars);
  Transcript tr(t);
  HashTranscript h(ht);
  HFr e;
  memcpy(&e, eval, 32);
  brakedown_verify(pp->p, root32, (const HFr*)point, num_vars, e, tr, h);
  LH_CATCH
}
lh_status lh_brakedown_batch_verify(const lh_brakedown_param* pp, size_t num_vars, const uint8_t* roots, size_t num_comms,
                                    const lh_fr* points, size_t num_points, const lh_evaluation* evals,
                                    size_t num_evals, lh_transcript* t, lh_hash_transcript* ht) {
  LH_TRY
  NEED(pp);
  NEED_N(roots, num_comms);
  NEED_N(points, num_points);
  NEED_N(evals, num_evals);
  Transcript tr(t);
  HashTranscript h(ht);
  for (size_t i = 0; i < num_evals; i++) {
    const lh_evaluation& e = evals[i];
    LH_REQUIRE(e.poly < num_comms && e.point < num_points, LH_ERR_ARG, "brakedown batch_verify: evaluation out of range");
    HFr v;
    memcpy(&v, &e.value, 32);
    brakedown_verify(pp->p, roots + 32 * (size_t)e.poly, (const HFr*)points + (size_t)e.point * num_vars, num_vars, v,
                     tr, h);
  }
  LH_CATCH
}

// HyperPlonk over Brakedown (brakedown.cpp brakedown_pcs; the verifier in verifier.cpp)
static std::vector<BdComm*> bd_comms_of(lh_brakedown_comm* const* comms, size_t n, const char* what) {
  LH_REQUIRE(comms != nullptr || n == 0, LH_ERR_ARG, std::string("null argument: ") + what);
  std::vector<BdComm*> v(n);
  for (size_t i = 0; i < n; i++) {
    LH_REQUIRE(comms[i], LH_ERR_ARG, std::string("null argument: ") + what + "[i]");
    v[i] = &comms[i]->c;
  }
  return v;
}
lh_status lh_hyperplonk_prove_brakedown(lh_ctx* ctx, const lh_brakedown_param* bp, const lh_hp_param* pp,
                                        lh_brakedown_comm* const* preprocess_comms,
                                        lh_brakedown_comm* const* permutation_comms, const lh_fr* const* instances,
                                        const lh_fr* const* d_witness_polys, lh_transcript* t, lh_hash_transcript* ht) {
  LH_TRY NEED_CTX(ctx);
  NEED(bp);
  NEED(pp);
  NEED_N(d_witness_polys, pp->num_witness_polys);
  NEED_N(instances, pp->num_instance_polys);
  const std::vector<BdComm*> pre = bd_comms_of(preprocess_comms, pp->num_preprocess_polys, "preprocess_comms"),
                             perm = bd_comms_of(permutation_comms, pp->num_permutation_polys, "permutation_comms");
  Transcript tr(t);
  HashTranscript h(ht);
  const HpPhases ph = hp_single_phase(*pp, (const Fr* const*)d_witness_polys);
  brakedown_hyperplonk_prove_phases(ctx->c, bp->p, *pp, pre.data(), perm.data(), ph, (const HFr* const*)instances, tr, h);
  LH_CATCH
}
lh_status lh_hyperplonk_prove_phases_brakedown(lh_ctx* ctx, const lh_brakedown_param* bp, const lh_hp_param* pp,
                                               lh_brakedown_comm* const* preprocess_comms,
                                               lh_brakedown_comm* const* permutation_comms, size_t num_phases,
                                               const size_t* num_witness_polys, const size_t* num_challenges,
                                               const lh_fr* const* instances, const lh_hp_circuit* circuit, lh_transcript* t,
                                               lh_hash_transcript* ht) {
  LH_TRY NEED_CTX(ctx);
  NEED(bp);
  NEED(pp);
  NEED(circuit);
  NEED_N(instances, pp->num_instance_polys);
  const std::vector<BdComm*> pre = bd_comms_of(preprocess_comms, pp->num_preprocess_polys, "preprocess_comms"),
                             perm = bd_comms_of(permutation_comms, pp->num_permutation_polys, "permutation_comms");
  Transcript tr(t);
  HashTranscript h(ht);
  const HpPhases ph = hp_phases_of(pp, num_phases, num_witness_polys, num_challenges, circuit);
  brakedown_hyperplonk_prove_phases(ctx->c, bp->p, *pp, pre.data(), perm.data(), ph, (const HFr* const*)instances, tr, h);
  LH_CATCH
}
lh_status lh_hyperplonk_verify_phases_brakedown(const lh_brakedown_param* bp, const lh_hp_vparam* hvp,
                                                const uint8_t* preprocess_roots, const uint8_t* permutation_roots,
                                                size_t num_phases, const size_t* num_witness_polys,
                                                const size_t* num_challenges, const lh_fr* const* instances, lh_transcript* t,
                                                lh_hash_transcript* ht) {
  LH_TRY
  NEED(bp);
  NEED(hvp);
  NEED_N(preprocess_roots, hvp->num_preprocess_polys);
  NEED_N(permutation_roots, hvp->num_permutation_polys);
  NEED_N(instances, hvp->num_instance_polys);
  const VerifierPhases ph = verifier_phases_of(num_phases, num_witness_polys, num_challenges);
  Transcript tr(t);
  HashTranscript h(ht);
  brakedown_hyperplonk_verify_phases(bp->p, *hvp, preprocess_roots, permutation_roots, ph.num_witness_polys, ph.num_challenges,
                                     (const HFr* const*)instances, tr, h);
  LH_CATCH
}
lh_status lh_hyperplonk_verify_brakedown(const lh_brakedown_param* bp, const lh_hp_vparam* hvp, const uint8_t* preprocess_roots,
                                         const uint8_t* permutation_roots, const lh_fr* const* instances, lh_transcript* t,
                                         lh_hash_transcript* ht) {
  if (!hvp) return lh_hyperplonk_verify_phases_brakedown(bp, hvp, preprocess_roots, permutation_roots, 0, nullptr, nullptr,
                                                         instances, t, ht);
  return lh_hyperplonk_verify_phases_brakedown(bp, hvp, preprocess_roots, permutation_roots, 1, &hvp->num_witness_polys,
                                               &hvp->num_challenges, instances, t, ht);
}

// Lasso over Brakedown (brakedown.cpp brakedown_lasso_prove; the verifier in verifier.cpp)
lh_status lh_lasso_prove_brakedown(lh_ctx* ctx, const lh_brakedown_param* bp, const lh_lasso_table* table, size_t num_vars,
                                   const uint32_t* const* d_dims, lh_transcript* t, lh_hash_transcript* ht) {
  LH_TRY NEED_CTX(ctx);
  NEED(bp);
  NEED(table);
  NEED(d_dims);
  Transcript tr(t);
  HashTranscript h(ht);
  brakedown_lasso_prove(ctx->c, bp->p, *table, num_vars, d_dims, tr, h);
  LH_CATCH
}
lh_status lh_lasso_verify_brakedown(const lh_brakedown_param* bp, const lh_lasso_table* table, size_t num_vars,
                                    lh_transcript* t, lh_hash_transcript* ht) {
  LH_TRY
  NEED(bp);
  NEED(table);
  Transcript tr(t);
  HashTranscript h(ht);
  brakedown_lasso_verify(bp->p, *table, num_vars, tr, h);
  lh_hash_transcript own;  // the built-in transcript knows where its stream ends (a caller's own checks that itself)
  if (keccak_transcript_hash_io(t, &own)) {
    const KeccakTranscript* k = (const KeccakTranscript*)t->user;
    if (k->pos != k->stream.size()) throw Error(LH_ERR_INVALID_SNARK, "trailing bytes in proof");
  }
  LH_CATCH
}

lh_status lh_lasso_prove_zeromorph(lh_ctx* ctx, const lh_usrs* srs, size_t poly_size, const lh_lasso_table* table,
                                   size_t num_vars, const uint32_t* const* d_dims, lh_transcript* t) {
  LH_TRY NEED_CTX(ctx);
  NEED(srs);
  lasso_prove_entry(ctx->c, table, num_vars, d_dims, t, [&] { return zeromorph_pcs(ctx->c, srs->s, poly_size); });
  LH_CATCH
}
lh_status lh_lasso_verify_zeromorph(const lh_zm_vp* vp, const lh_lasso_table* table, size_t num_vars, lh_transcript* t) {
  LH_TRY
  NEED(vp);
  lasso_verify_entry(table, num_vars, t, [&] { return zeromorph_verifier(*vp->p); });
  LH_CATCH
}
lh_status lh_hyperplonk_prove_zeromorph(lh_ctx* ctx, const lh_usrs* srs, size_t poly_size, const lh_hp_param* pp,
                                        const lh_fr* const* instances, const lh_fr* const* d_witness_polys,
                                        lh_transcript* t) {
  LH_TRY NEED_CTX(ctx);
  NEED(srs);
  hyperplonk_prove_entry(ctx->c, pp, instances, d_witness_polys, t, [&] { return zeromorph_pcs(ctx->c, srs->s, poly_size); });
  LH_CATCH
}
lh_status lh_hyperplonk_verify_zeromorph(const lh_zm_vp* vp, const lh_hp_vparam* hvp, const lh_fr* const* instances,
                                         lh_transcript* t) {
  LH_TRY
  NEED(vp);
  hyperplonk_verify_entry(hvp, instances, t, [&] { return zeromorph_verifier(*vp->p); });
  LH_CATCH
}

lh_status lh_hyperplonk_prove_phases_zeromorph(lh_ctx* ctx, const lh_usrs* srs, size_t poly_size, const lh_hp_param* pp,
                                               size_t num_phases, const size_t* num_witness_polys,
                                               const size_t* num_challenges, const lh_fr* const* instances,
                                               const lh_hp_circuit* circuit, lh_transcript* t) {
  LH_TRY NEED_CTX(ctx);
  NEED(srs);
  hyperplonk_prove_phases_entry(ctx->c, pp, num_phases, num_witness_polys, num_challenges, instances, circuit, t,
                                [&] { return zeromorph_pcs(ctx->c, srs->s, poly_size); });
  LH_CATCH
}
lh_status lh_hyperplonk_verify_phases_zeromorph(const lh_zm_vp* vp, const lh_hp_vparam* hvp, size_t num_phases,
                                                const size_t* num_witness_polys, const size_t* num_challenges,
                                                const lh_fr* const* instances, lh_transcript* t) {
  LH_TRY
  NEED(vp);
  hyperplonk_verify_phases_entry(hvp, num_phases, num_witness_polys, num_challenges, instances, t,
                                 [&] { return zeromorph_verifier(*vp->p); });
  LH_CATCH
}

// ---------------------------------------------------------------- univariate KZG on its own, Gemini over it
static std::vector<UPoly> upolys_of(const lh_fr* const* d_polys, const size_t* lens, size_t num_polys) {
  std::vector<UPoly> polys(num_polys);
  for (size_t i = 0; i < num_polys; i++) {
    LH_REQUIRE(d_polys[i] != nullptr || lens[i] == 0, LH_ERR_ARG, "null argument: d_polys[i]");
    polys[i] = UPoly{(const Fr*)d_polys[i], lens[i]};
  }
  return polys;
}
lh_status lh_ukzg_batch_commit(lh_ctx* ctx, const lh_usrs* srs, size_t poly_size, const lh_fr* const* d_polys,
                               const size_t* lens, size_t num_polys, lh_g1* out_comms) {
  LH_TRY NEED_CTX(ctx);
  NEED(srs);
  NEED_N(d_polys, num_polys);
  NEED_N(lens, num_polys);
  NEED_N(out_comms, num_polys);
  const std::vector<UPoly> polys = upolys_of(d_polys, lens, num_polys);
  std::vector<HG1> c = ukzg_batch_commit(ctx->c, srs->s, poly_size, polys.data(), num_polys);
  if (num_polys) memcpy(out_comms, c.data(), 64 * num_polys);
  LH_CATCH
}
lh_status lh_ukzg_open(lh_ctx* ctx, const lh_usrs* srs, size_t poly_size, const lh_fr* d_poly, size_t len,
                       const lh_fr* point, lh_transcript* t) {
  LH_TRY NEED_CTX(ctx);
  NEED(srs);
  NEED_N(d_poly, len);
  NEED(point);
  Transcript tr(t);
  HFr x;
  memcpy(&x, point, 32);
  ukzg_open(ctx->c, srs->s, poly_size, UPoly{(const Fr*)d_poly, len}, x, tr);
  LH_CATCH
}
lh_status lh_ukzg_batch_open(lh_ctx* ctx, const lh_usrs* srs, size_t poly_size, const lh_fr* const* d_polys,
                             const size_t* lens, size_t num_polys, const lh_fr* points, size_t num_points,
                             const lh_evaluation* evals, size_t num_evals, lh_transcript* t) {
  LH_TRY NEED_CTX(ctx);
  NEED(srs);
  NEED_N(d_polys, num_polys);
  NEED_N(lens, num_polys);
  NEED_N(points, num_points);
  NEED_N(evals, num_evals);
  Transcript tr(t);
  const std::vector<UPoly> polys = upolys_of(d_polys, lens, num_polys);
  ukzg_batch_open(ctx->c, srs->s, poly_size, polys.data(), num_polys, (const HFr*)points, num_points, evals, num_evals, tr);
  LH_CATCH
}
lh_status lh_ukzg_vp_setup(const lh_fr* s, lh_ukzg_vp** out) {
  LH_TRY
  NEED(s);
  NEED(out);
  HFr sv;
  memcpy(&sv, s, 32);
  *out = new lh_ukzg_vp{ukzg_vp_setup(sv)};
  LH_CATCH
}
lh_status lh_ukzg_vp_new(const lh_g1* g1, const lh_g2* g2, const lh_g2* s_g2, lh_ukzg_vp** out) {
  LH_TRY
  NEED(g1);
  NEED(g2);
  NEED(s_g2);
  NEED(out);
  *out = new lh_ukzg_vp{ukzg_vp_new(*g1, *g2, *s_g2)};
  LH_CATCH
}
lh_status lh_ukzg_vp_export(const lh_ukzg_vp* vp, lh_g1* g1, lh_g2* g2, lh_g2* s_g2) {
  LH_TRY
  NEED(vp);
  NEED(g1);
  NEED(g2);
  NEED(s_g2);
  ukzg_vp_export(*vp->p, g1, g2, s_g2);
  LH_CATCH
}
void lh_ukzg_vp_free(lh_ukzg_vp* vp) {
  if (!vp) return;
  ukzg_vp_free(vp->p);
  delete vp;
}
lh_status lh_ukzg_verify(const lh_ukzg_vp* vp, const lh_g1* comm, const lh_fr* point, const lh_fr* eval, lh_transcript* t) {
  LH_TRY
  NEED(vp);
  NEED(comm);
  NEED(point);
  NEED(eval);
  Transcript tr(t);
  HG1 c;
  memcpy(&c, comm, sizeof(c));
  HFr x, e;
  memcpy(&x, point, 32);
  memcpy(&e, eval, 32);
  ukzg_verify(*vp->p, c, x, e, tr);
  LH_CATCH
}
lh_status lh_ukzg_batch_verify(const lh_ukzg_vp* vp, const lh_g1* comms, size_t num_comms, const lh_fr* points,
                               size_t num_points, const lh_evaluation* evals, size_t num_evals, lh_transcript* t) {
  LH_TRY
  NEED(vp);
  NEED_N(comms, num_comms);
  NEED_N(points, num_points);
  NEED_N(evals, num_evals);
  Transcript tr(t);
  ukzg_batch_verify(*vp->p, (const HG1*)comms, num_comms, (const HFr*)points, num_points, evals, num_evals, tr);
  LH_CATCH
}
lh_status lh_gemini_batch_commit(lh_ctx* ctx, const lh_usrs* srs, size_t poly_size, const lh_fr* const* d_polys,
                                 size_t num_polys, size_t num_vars, lh_g1* out_comms) {
  LH_TRY NEED_CTX(ctx);
  NEED(srs);
  NEED_N(d_polys, num_polys);
  NEED_N(out_comms, num_polys);
  for (size_t i = 0; i < num_polys; i++) NEED(d_polys[i]);
  std::vector<HG1> c = gemini_batch_commit(ctx->c, srs->s, poly_size, (const Fr* const*)d_polys, num_polys, num_vars);
  if (num_polys) memcpy(out_comms, c.data(), 64 * num_polys);
  LH_CATCH
}
lh_status lh_gemini_open(lh_ctx* ctx, const lh_usrs* srs, size_t poly_size, const lh_fr* d_poly, size_t num_vars,
                         const lh_fr* point, lh_transcript* t) {
  LH_TRY NEED_CTX(ctx);
  NEED(srs);
  NEED(d_poly);
  NEED_N(point, num_vars);
  Transcript tr(t);
  gemini_open(ctx->c, srs->s, poly_size, (const Fr*)d_poly, num_vars, (const HFr*)point, tr);
  LH_CATCH
}
lh_status lh_gemini_batch_open(lh_ctx* ctx, const lh_usrs* srs, size_t poly_size, size_t num_vars,
                               const lh_fr* const* d_polys, size_t num_polys, const lh_fr* points, size_t num_points,
                               const lh_evaluation* evals, size_t num_evals, lh_transcript* t) {
  LH_TRY NEED_CTX(ctx);
  NEED(srs);
  NEED_N(d_polys, num_polys);
  NEED_N(points, num_points);
  NEED_N(evals, num_evals);
  Transcript tr(t);
  gemini_batch_open(ctx->c, srs->s, poly_size, num_vars, (const Fr* const*)d_polys, num_polys, (const HFr*)points,
                    num_points, evals, num_evals, tr);
  LH_CATCH
}
lh_status lh_gemini_folds(lh_ctx* ctx, const lh_fr* d_poly, size_t num_vars, const lh_fr* point, lh_fr* d_out) {
  LH_TRY NEED_CTX(ctx);
  NEED(d_poly);
  NEED_N(point, num_vars);
  NEED_N(d_out, num_vars > 1);
  gemini_folds(ctx->c, (const Fr*)d_poly, num_vars, (const HFr*)point, (Fr*)d_out);
  ctx->c.sync();
  LH_CATCH
}
lh_status lh_gemini_verify(const lh_ukzg_vp* vp, const lh_g1* comm, const lh_fr* point, size_t num_vars,
                           const lh_fr* eval, lh_transcript* t) {
  LH_TRY
  NEED(vp);
  NEED(comm);
  NEED(eval);
  NEED_N(point, num_vars);
  Transcript tr(t);
  HG1 c;
  memcpy(&c, comm, sizeof(c));
  HFr e;
  memcpy(&e, eval, 32);
  gemini_verify(*vp->p, c, (const HFr*)point, num_vars, e, tr);
  LH_CATCH
}
lh_status lh_gemini_batch_verify(const lh_ukzg_vp* vp, size_t num_vars, const lh_g1* comms, size_t num_comms,
                                 const lh_fr* points, size_t num_points, const lh_evaluation* evals, size_t num_evals,
                                 lh_transcript* t) {
  LH_TRY
  NEED(vp);
  NEED_N(comms, num_comms);
  NEED_N(points, num_points);
  NEED_N(evals, num_evals);
  Transcript tr(t);
  gemini_batch_verify(*vp->p, num_vars, (const HG1*)comms, num_comms, (const HFr*)points, num_points, evals, num_evals, tr);
  LH_CATCH
}
lh_status lh_lasso_prove_gemini(lh_ctx* ctx, const lh_usrs* srs, size_t poly_size, const lh_lasso_table* table,
                                size_t num_vars, const uint32_t* const* d_dims, lh_transcript* t) {
  LH_TRY NEED_CTX(ctx);
  NEED(srs);
  lasso_prove_entry(ctx->c, table, num_vars, d_dims, t, [&] { return gemini_pcs(ctx->c, srs->s, poly_size); });
  LH_CATCH
}
lh_status lh_lasso_verify_gemini(const lh_ukzg_vp* vp, const lh_lasso_table* table, size_t num_vars, lh_transcript* t) {
  LH_TRY
  NEED(vp);
  lasso_verify_entry(table, num_vars, t, [&] { return gemini_verifier(*vp->p); });
  LH_CATCH
}
lh_status lh_hyperplonk_prove_gemini(lh_ctx* ctx, const lh_usrs* srs, size_t poly_size, const lh_hp_param* pp,
                                     const lh_fr* const* instances, const lh_fr* const* d_witness_polys, lh_transcript* t) {
  LH_TRY NEED_CTX(ctx);
  NEED(srs);
  hyperplonk_prove_entry(ctx->c, pp, instances, d_witness_polys, t, [&] { return gemini_pcs(ctx->c, srs->s, poly_size); });
  LH_CATCH
}
lh_status lh_hyperplonk_verify_gemini(const lh_ukzg_vp* vp, const lh_hp_vparam* hvp, const lh_fr* const* instances,
                                      lh_transcript* t) {
  LH_TRY
  NEED(vp);
  hyperplonk_verify_entry(hvp, instances, t, [&] { return gemini_verifier(*vp->p); });
  LH_CATCH
}
lh_status lh_hyperplonk_prove_phases_gemini(lh_ctx* ctx, const lh_usrs* srs, size_t poly_size, const lh_hp_param* pp,
                                            size_t num_phases, const size_t* num_witness_polys, const size_t* num_challenges,
                                            const lh_fr* const* instances, const lh_hp_circuit* circuit, lh_transcript* t) {
  LH_TRY NEED_CTX(ctx);
  NEED(srs);
  hyperplonk_prove_phases_entry(ctx->c, pp, num_phases, num_witness_polys, num_challenges, instances, circuit, t,
                                [&] { return gemini_pcs(ctx->c, srs->s, poly_size); });
  LH_CATCH
}
lh_status lh_hyperplonk_verify_phases_gemini(const lh_ukzg_vp* vp, const lh_hp_vparam* hvp, size_t num_phases,
                                             const size_t* num_witness_polys, const size_t* num_challenges,
                                             const lh_fr* const* instances, lh_transcript* t) {
  LH_TRY
  NEED(vp);
  hyperplonk_verify_phases_entry(hvp, num_phases, num_witness_polys, num_challenges, instances, t,
                                 [&] { return gemini_verifier(*vp->p); });
  LH_CATCH
}

// ---------------------------------------------------------------- the multilinear IPA over bn256::G1Affine
lh_status lh_ipa_setup(lh_ctx* ctx, size_t poly_size, lh_ipa_param** out) {
  LH_TRY
  NEED(out);
  OnDevice on(ctx ? ctx->c.device : -1);
  *out = new lh_ipa_param{ipa_setup(ctx ? &ctx->c : nullptr, poly_size)};
  LH_CATCH
}
void lh_ipa_param_free(lh_ctx* ctx, lh_ipa_param* param) {
  if (!param) return;
  if (ctx) (void)hipStreamSynchronize(ctx->c.stream);
  delete param;
}
size_t lh_ipa_param_size(const lh_ipa_param* param) { return param ? (size_t)1 << param->p->num_vars : 0; }
lh_status lh_ipa_param_download(lh_ctx* ctx, const lh_ipa_param* param, lh_g1* g, lh_g1* h) {
  LH_TRY
  NEED(param);
  const size_t size = (size_t)1 << param->p->num_vars;
  if (g) {
    if (param->p->d_g) {
      NEED_CTX(ctx);
      LH_HIP(hipMemcpyAsync(g, param->p->d_g, size * sizeof(G1Affine), hipMemcpyDeviceToHost, ctx->c.stream));
      ctx->c.sync();
    } else {
      memcpy(g, ipa_host_g(*param->p).data(), size * sizeof(HG1));
    }
  }
  if (h) memcpy(h, &param->p->h, sizeof(HG1));
  LH_CATCH
}
lh_status lh_ipa_batch_commit(lh_ctx* ctx, const lh_ipa_param* param, size_t poly_size, const lh_fr* const* d_polys,
                              size_t num_polys, size_t num_vars, lh_g1* out_comms) {
  LH_TRY NEED_CTX(ctx);
  NEED(param);
  NEED_N(d_polys, num_polys);
  NEED_N(out_comms, num_polys);
  for (size_t i = 0; i < num_polys; i++) NEED(d_polys[i]);
  std::vector<HG1> c = ipa_batch_commit(ctx->c, *param->p, poly_size, (const Fr* const*)d_polys, num_polys, num_vars);
  if (num_polys) memcpy(out_comms, c.data(), 64 * num_polys);
  LH_CATCH
}
lh_status lh_ipa_open(lh_ctx* ctx, const lh_ipa_param* param, size_t poly_size, const lh_fr* d_poly, size_t num_vars,
                      const lh_fr* point, lh_transcript* t) {
  LH_TRY NEED_CTX(ctx);
  NEED(param);
  NEED(d_poly);
  NEED_N(point, num_vars);
  Transcript tr(t);
  ipa_open(ctx->c, *param->p, poly_size, (const Fr*)d_poly, num_vars, (const HFr*)point, tr);
  LH_CATCH
}
lh_status lh_ipa_batch_open(lh_ctx* ctx, const lh_ipa_param* param, size_t poly_size, size_t num_vars,
                            const lh_fr* const* d_polys, size_t num_polys, const lh_fr* points, size_t num_points,
                            const lh_evaluation* evals, size_t num_evals, lh_transcript* t) {
  LH_TRY NEED_CTX(ctx);
  NEED(param);
  NEED_N(d_polys, num_polys);
  NEED_N(points, num_points);
  NEED_N(evals, num_evals);
  for (size_t i = 0; i < num_polys; i++) NEED(d_polys[i]);
  Transcript tr(t);
  ipa_batch_open(ctx->c, *param->p, poly_size, num_vars, (const Fr* const*)d_polys, num_polys, (const HFr*)points, num_points,
                 evals, num_evals, tr);
  LH_CATCH
}
lh_status lh_ipa_verify(const lh_ipa_param* param, size_t poly_size, const lh_g1* comm, const lh_fr* point, size_t num_vars,
                        const lh_fr* eval, lh_transcript* t) {
  LH_TRY
  NEED(param);
  NEED(comm);
  NEED(eval);
  NEED_N(point, num_vars);
  Transcript tr(t);
  HG1 c;
  memcpy(&c, comm, sizeof(c));
  HFr e;
  memcpy(&e, eval, 32);
  ipa_verify(*param->p, poly_size, c, (const HFr*)point, num_vars, e, tr);
  LH_CATCH
}
lh_status lh_ipa_batch_verify(const lh_ipa_param* param, size_t poly_size, size_t num_vars, const lh_g1* comms, size_t num_comms,
                              const lh_fr* points, size_t num_points, const lh_evaluation* evals, size_t num_evals,
                              lh_transcript* t) {
  LH_TRY
  NEED(param);
  NEED_N(comms, num_comms);
  NEED_N(points, num_points);
  NEED_N(evals, num_evals);
  Transcript tr(t);
  ipa_batch_verify(*param->p, poly_size, num_vars, (const HG1*)comms, num_comms, (const HFr*)points, num_points, evals, num_evals,
                   tr);
  LH_CATCH
}
lh_status lh_g1_axpy(lh_ctx* ctx, const lh_g1* d_a, const lh_g1* d_b, size_t n, const lh_fr* s, lh_g1* d_out) {
  LH_TRY NEED_CTX(ctx);
  NEED_N(d_a, n);
  NEED_N(d_b, n);
  NEED_N(d_out, n);
  NEED(s);
  Fr sv;
  memcpy(&sv, s, 32);
  k_g1_axpy(ctx->c, (const G1Affine*)d_a, (const G1Affine*)d_b, n, sv, (G1Affine*)d_out);
  ctx->c.sync();
  LH_CATCH
}
lh_status lh_g1_rows_msm(lh_ctx* ctx, const void* d_scalars, int scalars_u32, uint32_t bits, size_t n, size_t row_len,
                         const lh_g1* d_bases, lh_g1* out_rows) {
  LH_TRY NEED_CTX(ctx);
  if (row_len == 0) throw Error(LH_ERR_ARG, "rows msm: row_len must be at least 1");
  NEED_N(d_scalars, n);
  NEED_N(d_bases, n);
  NEED_N(out_rows, n);
  k_g1_rows_msm(ctx->c, d_scalars, scalars_u32 != 0, bits, n, row_len, (const G1Affine*)d_bases, nullptr, 0, 0, (G1Affine*)out_rows);
  LH_CATCH
}
// ---------------------------------------------------------------- Hyrax on top of the IPA
lh_status lh_hyrax_setup(lh_ctx* ctx, size_t poly_size, size_t batch_size, lh_ipa_param** out) {
  LH_TRY
  NEED(out);
  const HyraxDims d = hyrax_dims(poly_size, batch_size);
  OnDevice on(ctx ? ctx->c.device : -1);
  *out = new lh_ipa_param{ipa_setup(ctx ? &ctx->c : nullptr, (size_t)1 << d.row_num_vars)};
  LH_CATCH
}
lh_status lh_hyrax_dims(size_t poly_size, size_t batch_size, size_t* num_vars, size_t* batch_num_vars, size_t* row_num_vars) {
  LH_TRY
  const HyraxDims d = hyrax_dims(poly_size, batch_size);
  if (num_vars) *num_vars = d.num_vars;
  if (batch_num_vars) *batch_num_vars = d.batch_num_vars;
  if (row_num_vars) *row_num_vars = d.row_num_vars;
  LH_CATCH
}
lh_status lh_hyrax_trim(const lh_ipa_param* param, size_t poly_size, size_t batch_size, size_t* row_num_vars, size_t* num_chunks) {
  LH_TRY
  NEED(param);
  const HyraxDims d = hyrax_trim(*param->p, poly_size, batch_size);
  if (row_num_vars) *row_num_vars = d.row_num_vars;
  if (num_chunks) *num_chunks = d.num_chunks();
  LH_CATCH
}
lh_status lh_hyrax_batch_commit(lh_ctx* ctx, const lh_ipa_param* param, size_t poly_size, size_t batch_size,
                                const lh_fr* const* d_polys, size_t num_polys, size_t num_vars, lh_g1* out_comms) {
  LH_TRY NEED_CTX(ctx);
  NEED(param);
  NEED_N(d_polys, num_polys);
  NEED_N(out_comms, num_polys);
  for (size_t i = 0; i < num_polys; i++) NEED(d_polys[i]);
  std::vector<HG1> c = hyrax_batch_commit(ctx->c, *param->p, poly_size, batch_size, (const Fr* const*)d_polys, num_polys, num_vars);
  if (!c.empty()) memcpy(out_comms, c.data(), 64 * c.size());
  LH_CATCH
}
lh_status lh_hyrax_open(lh_ctx* ctx, const lh_ipa_param* param, size_t poly_size, size_t batch_size, const lh_fr* d_poly,
                        size_t num_vars, const lh_fr* point, lh_transcript* t) {
  LH_TRY NEED_CTX(ctx);
  NEED(param);
  NEED(d_poly);
  NEED_N(point, num_vars);
  Transcript tr(t);
  hyrax_open(ctx->c, *param->p, poly_size, batch_size, (const Fr*)d_poly, num_vars, (const HFr*)point, tr);
  LH_CATCH
}
lh_status lh_hyrax_batch_open(lh_ctx* ctx, const lh_ipa_param* param, size_t poly_size, size_t batch_size, size_t num_vars,
                              const lh_fr* const* d_polys, size_t num_polys, const lh_fr* points, size_t num_points,
                              const lh_evaluation* evals, size_t num_evals, lh_transcript* t) {
  LH_TRY NEED_CTX(ctx);
  NEED(param);
  NEED_N(d_polys, num_polys);
  NEED_N(points, num_points);
  NEED_N(evals, num_evals);
  for (size_t i = 0; i < num_polys; i++) NEED(d_polys[i]);
  Transcript tr(t);
  hyrax_batch_open(ctx->c, *param->p, poly_size, batch_size, num_vars, (const Fr* const*)d_polys, num_polys, (const HFr*)points,
                   num_points, evals, num_evals, tr);
  LH_CATCH
}
lh_status lh_hyrax_verify(const lh_ipa_param* param, size_t poly_size, size_t batch_size, const lh_g1* comm, const lh_fr* point,
                          size_t num_vars, const lh_fr* eval, lh_transcript* t) {
  LH_TRY
  NEED(param);
  NEED(comm);
  NEED(eval);
  NEED_N(point, num_vars);
  Transcript tr(t);
  HFr e;
  memcpy(&e, eval, 32);
  hyrax_verify(*param->p, poly_size, batch_size, (const HG1*)comm, (const HFr*)point, num_vars, e, tr);
  LH_CATCH
}
lh_status lh_hyrax_batch_verify(const lh_ipa_param* param, size_t poly_size, size_t batch_size, size_t num_vars,
                                const lh_g1* comms, size_t num_comms, const lh_fr* points, size_t num_points,
                                const lh_evaluation* evals, size_t num_evals, lh_transcript* t) {
  LH_TRY
  NEED(param);
  NEED_N(comms, num_comms);
  NEED_N(points, num_points);
  NEED_N(evals, num_evals);
  Transcript tr(t);
  hyrax_batch_verify(*param->p, poly_size, batch_size, num_vars, (const HG1*)comms, num_comms, (const HFr*)points, num_points,
                     evals, num_evals, tr);
  LH_CATCH
}
lh_status lh_lasso_prove_hyrax(lh_ctx* ctx, const lh_ipa_param* param, size_t poly_size, size_t batch_size,
                               const lh_lasso_table* table, size_t num_vars, const uint32_t* const* d_dims, lh_transcript* t) {
  LH_TRY NEED_CTX(ctx);
  NEED(param);
  lasso_prove_entry(ctx->c, table, num_vars, d_dims, t, [&] {
    hyrax_lasso_vars(*param->p, poly_size, batch_size, *table, num_vars);
    return hyrax_pcs(ctx->c, *param->p, poly_size, batch_size);
  });
  LH_CATCH
}
lh_status lh_lasso_verify_hyrax(const lh_ipa_param* param, size_t poly_size, size_t batch_size, const lh_lasso_table* table,
                                size_t num_vars, lh_transcript* t) {
  LH_TRY
  NEED(param);
  lasso_verify_entry(table, num_vars, t, [&] {
    hyrax_lasso_vars(*param->p, poly_size, batch_size, *table, num_vars);
    return hyrax_verifier(*param->p, poly_size, batch_size);
  });
  LH_CATCH
}
lh_status lh_hyperplonk_prove_hyrax(lh_ctx* ctx, const lh_ipa_param* param, size_t poly_size, size_t batch_size,
                                    const lh_hp_param* pp, const lh_fr* const* instances, const lh_fr* const* d_witness_polys,
                                    lh_transcript* t) {
  LH_TRY NEED_CTX(ctx);
  NEED(param);
  hyperplonk_prove_entry(ctx->c, pp, instances, d_witness_polys, t, [&] {
    hyrax_hyperplonk_vars(*param->p, poly_size, batch_size, pp->num_vars);
    return hyrax_pcs(ctx->c, *param->p, poly_size, batch_size);
  });
  LH_CATCH
}
lh_status lh_hyperplonk_verify_hyrax(const lh_ipa_param* param, size_t poly_size, size_t batch_size, const lh_hp_vparam* hvp,
                                     const lh_fr* const* instances, lh_transcript* t) {
  LH_TRY
  NEED(param);
  hyperplonk_verify_entry(hvp, instances, t, [&] {
    hyrax_hyperplonk_vars(*param->p, poly_size, batch_size, hvp->num_vars);
    return hyrax_verifier(*param->p, poly_size, batch_size);
  });
  LH_CATCH
}
lh_status lh_hyperplonk_prove_phases_hyrax(lh_ctx* ctx, const lh_ipa_param* param, size_t poly_size, size_t batch_size,
                                           const lh_hp_param* pp, size_t num_phases, const size_t* num_witness_polys,
                                           const size_t* num_challenges, const lh_fr* const* instances,
                                           const lh_hp_circuit* circuit, lh_transcript* t) {
  LH_TRY NEED_CTX(ctx);
  NEED(param);
  hyperplonk_prove_phases_entry(
      ctx->c, pp, num_phases, num_witness_polys, num_challenges, instances, circuit, t,
      [&] { return hyrax_pcs(ctx->c, *param->p, poly_size, batch_size); },
      [&] { hyrax_hyperplonk_vars(*param->p, poly_size, batch_size, pp->num_vars); });
  LH_CATCH
}
lh_status lh_hyperplonk_verify_phases_hyrax(const lh_ipa_param* param, size_t poly_size, size_t batch_size, const lh_hp_vparam* hvp,
                                            size_t num_phases, const size_t* num_witness_polys, const size_t* num_challenges,
                                            const lh_fr* const* instances, lh_transcript* t) {
  LH_TRY
  NEED(param);
  hyperplonk_verify_phases_entry(hvp, num_phases, num_witness_polys, num_challenges, instances, t, [&] {
    hyrax_hyperplonk_vars(*param->p, poly_size, batch_size, hvp->num_vars);
    return hyrax_verifier(*param->p, poly_size, batch_size);
  });
  LH_CATCH
}
lh_status lh_lasso_prove_ipa(lh_ctx* ctx, const lh_ipa_param* param, size_t poly_size, const lh_lasso_table* table,
                             size_t num_vars, const uint32_t* const* d_dims, lh_transcript* t) {
  LH_TRY NEED_CTX(ctx);
  NEED(param);
  lasso_prove_entry(ctx->c, table, num_vars, d_dims, t, [&] { return ipa_pcs(ctx->c, *param->p, poly_size); });
  LH_CATCH
}
lh_status lh_lasso_verify_ipa(const lh_ipa_param* param, size_t poly_size, const lh_lasso_table* table, size_t num_vars,
                              lh_transcript* t) {
  LH_TRY
  NEED(param);
  lasso_verify_entry(table, num_vars, t, [&] { return ipa_verifier(*param->p, poly_size); });
  LH_CATCH
}
lh_status lh_hyperplonk_prove_ipa(lh_ctx* ctx, const lh_ipa_param* param, size_t poly_size, const lh_hp_param* pp,
                                  const lh_fr* const* instances, const lh_fr* const* d_witness_polys, lh_transcript* t) {
  LH_TRY NEED_CTX(ctx);
  NEED(param);
  hyperplonk_prove_entry(ctx->c, pp, instances, d_witness_polys, t, [&] { return ipa_pcs(ctx->c, *param->p, poly_size); });
  LH_CATCH
}
lh_status lh_hyperplonk_verify_ipa(const lh_ipa_param* param, size_t poly_size, const lh_hp_vparam* hvp,
                                   const lh_fr* const* instances, lh_transcript* t) {
  LH_TRY
  NEED(param);
  hyperplonk_verify_entry(hvp, instances, t, [&] { return ipa_verifier(*param->p, poly_size); });
  LH_CATCH
}
lh_status lh_hyperplonk_prove_phases_ipa(lh_ctx* ctx, const lh_ipa_param* param, size_t poly_size, const lh_hp_param* pp,
                                         size_t num_phases, const size_t* num_witness_polys, const size_t* num_challenges,
                                         const lh_fr* const* instances, const lh_hp_circuit* circuit, lh_transcript* t) {
  LH_TRY NEED_CTX(ctx);
  NEED(param);
  hyperplonk_prove_phases_entry(ctx->c, pp, num_phases, num_witness_polys, num_challenges, instances, circuit, t,
                                [&] { return ipa_pcs(ctx->c, *param->p, poly_size); });
  LH_CATCH
}
lh_status lh_hyperplonk_verify_phases_ipa(const lh_ipa_param* param, size_t poly_size, const lh_hp_vparam* hvp, size_t num_phases,
                                          const size_t* num_witness_polys, const size_t* num_challenges,
                                          const lh_fr* const* instances, lh_transcript* t) {
  LH_TRY
  NEED(param);
  hyperplonk_verify_phases_entry(hvp, num_phases, num_witness_polys, num_challenges, instances, t,
                                 [&] { return ipa_verifier(*param->p, poly_size); });
  LH_CATCH
}

lh_status lh_debug_jit_source(const uint32_t* code, size_t num_instrs, uint32_t num_regs, uint32_t result_reg, int degree,
                              char* out, size_t cap, size_t* len) {
  LH_TRY
  NEED(code);
  NEED(len);
  LH_REQUIRE(num_regs >= 1 && num_regs <= 16 && result_reg < num_regs && degree >= 1, LH_ERR_ARG, "jit source: bad program header");
  const std::string src = lh::jit_debug_source(code, num_instrs, num_regs, result_reg, degree);
  *len = src.size();
  if (out && cap) {
    const size_t n = std::min(cap - 1, src.size());
    memcpy(out, src.data(), n);
    out[n] = 0;
  }
  LH_CATCH
}

// (development) the radix sort and the Lasso access counters on their own: tests/test_gpu_sort.py
lh_status lh_debug_sort_pairs(lh_ctx* ctx, int key_bytes, const lh_debug_sort_slab* slabs, size_t count) {
  LH_TRY NEED_CTX(ctx);
  NEED_N(slabs, count);
  LH_REQUIRE(key_bytes == 4 || key_bytes == 8, LH_ERR_ARG, "debug sort: key_bytes is 4 or 8");
  LH_REQUIRE(key_bytes == 4 || count == 1, LH_ERR_ARG, "debug sort: u64 keys sort one slab per call");
  // (a shift by the key width or more is undefined in the kernels: refused here, before anything is launched)
  for (size_t i = 0; i < count; i++) {
    const lh_debug_sort_slab& s = slabs[i];
    LH_REQUIRE(s.bits >= 1 && s.bits <= 8u * key_bytes && s.first_bit <= 8u * key_bytes - s.bits, LH_ERR_ARG,
               "debug sort: the sorted bits [first_bit, first_bit + bits) must be a non-empty range inside the key");
    LH_REQUIRE(key_bytes == 4 || s.first_bit == 0, LH_ERR_ARG, "debug sort: u64 keys sort from bit 0");
    LH_REQUIRE(s.n == 0 || (s.d_keys_in && s.d_keys_out && s.d_vals_out), LH_ERR_ARG, "null argument: sort slab buffers");
    LH_REQUIRE(s.n < ((size_t)1 << 32), LH_ERR_ARG, "debug sort: too many pairs");
  }
  ArenaScope scope(ctx->c.arena);
  if (key_bytes == 4) {
    std::vector<SortSlab> v(count);
    for (size_t i = 0; i < count; i++)
      v[i] = SortSlab{(const uint32_t*)slabs[i].d_keys_in, (uint32_t*)slabs[i].d_keys_out, slabs[i].d_vals_in,
                      slabs[i].d_vals_out, slabs[i].n, slabs[i].bits, slabs[i].first_bit};
    sort_pairs_u32_batched(ctx->c, v.data(), count);
  } else {
    sort_pairs_u64(ctx->c, (const uint64_t*)slabs[0].d_keys_in, (uint64_t*)slabs[0].d_keys_out, slabs[0].d_vals_in,
                   slabs[0].d_vals_out, slabs[0].n, slabs[0].bits);
  }
  ctx->c.sync();
  LH_CATCH
}
lh_status lh_debug_lasso_counters(lh_ctx* ctx, const uint32_t* const* d_dims, size_t num_cols, size_t n, size_t m,
                                  uint32_t* const* d_read_ts, uint32_t* const* d_final_cts, uint32_t* const* d_keep_sorted,
                                  uint32_t* const* d_keep_index) {
  LH_TRY NEED_CTX(ctx);
  NEED(d_dims);
  NEED(d_read_ts);
  NEED(d_final_cts);
  LH_REQUIRE(num_cols >= 1 && num_cols <= (size_t)LH_LASSO_MAX_CHUNKS, LH_ERR_ARG, "debug counters: bad column count");
  LH_REQUIRE(m >= 1 && m <= ((size_t)1 << 32) && n < ((size_t)1 << 32), LH_ERR_ARG, "debug counters: bad shape");
  for (size_t j = 0; j < num_cols; j++) {
    LH_REQUIRE(d_final_cts[j] && (n == 0 || (d_dims[j] && d_read_ts[j])), LH_ERR_ARG, "null argument: counter columns");
    LH_REQUIRE(n == 0 || ((!d_keep_sorted || d_keep_sorted[j]) && (!d_keep_index || d_keep_index[j])), LH_ERR_ARG,
               "null argument: keep_sorted / keep_index column");
  }
  k_lasso_counters(ctx->c, d_dims, num_cols, n, m, d_read_ts, d_final_cts, d_keep_sorted, d_keep_index);
  ctx->c.sync();
  LH_CATCH
}
lh_status lh_debug_memcheck_witness(lh_ctx* ctx, const lh_memcheck_trace* trace, size_t num_vars, size_t mem_vars,
                                    const uint32_t* init, uint32_t* d_rt, uint32_t* d_fv, uint32_t* d_ft, uint32_t* d_m, int* out_bad) {
  LH_TRY NEED_CTX(ctx);
  NEED(trace);
  NEED(d_rt);
  NEED(d_fv);
  NEED(d_ft);
  NEED(d_m);
  NEED(out_bad);
  *out_bad = memcheck_witness(ctx->c, *trace, num_vars, mem_vars, init, d_rt, d_fv, d_ft, d_m) ? 0 : 1;
  LH_CATCH
}
lh_status lh_debug_spark_e(lh_ctx* ctx, size_t num_vars, size_t dim_vars, size_t num_dims, const uint32_t* const* d_dims,
                           const lh_fr* d_val, const lh_fr* point, lh_fr* const* d_E, lh_fr* out_value) {
  LH_TRY
  spark_check(num_vars, dim_vars, num_dims);
  NEED_CTX(ctx);
  NEED(out_value);
  const HFr v = spark_debug_e(ctx->c, num_vars, dim_vars, num_dims, d_dims, (const Fr*)d_val, (const HFr*)point, (Fr* const*)d_E);
  memcpy(out_value, &v, 32);
  LH_CATCH
}
lh_status lh_debug_spartan_spmv(lh_ctx* ctx, const lh_r1cs_key* key, int direction, const lh_fr* d_x, lh_fr* const d_out[3]) {
  LH_TRY NEED_CTX(ctx);
  NEED(key);
  spartan_debug_spmv(ctx->c, *(const R1csKey*)key, direction, (const Fr*)d_x, (Fr* const*)d_out);
  LH_CATCH
}
lh_status lh_debug_nova_spmv2(lh_ctx* ctx, const lh_r1cs_key* key, int direction, const lh_fr* d_x1, const lh_fr* d_x2,
                              lh_fr* const d_out1[3], lh_fr* const d_out2[3]) {
  LH_TRY NEED_CTX(ctx);
  NEED(key);
  nova_debug_spmv2(ctx->c, *(const R1csKey*)key, direction, (const Fr*)d_x1, (const Fr*)d_x2, (Fr* const*)d_out1, (Fr* const*)d_out2);
  LH_CATCH
}
lh_status lh_debug_nova_cross_term(lh_ctx* ctx, size_t dim_vars, const lh_fr* const d_mz1[3], const lh_fr* const d_mz2[3],
                                   const lh_fr* d_e1, const lh_fr* d_e2, const lh_fr* u1, const lh_fr* u2, lh_fr* d_t, size_t out_bad[2]) {
  LH_TRY NEED_CTX(ctx);
  NEED(d_mz1);
  NEED(d_mz2);
  NEED(u1);
  NEED(u2);
  NEED(d_t);
  NEED(out_bad);
  LH_REQUIRE(dim_vars >= 1 && dim_vars <= (size_t)LH_SPARTAN_MAX_DIM_VARS, LH_ERR_ARG, "nova: dim_vars out of range");
  lh::NovaCross p;
  for (int m = 0; m < 3; m++) p.mz1[m] = (const Fr*)d_mz1[m], p.mz2[m] = (const Fr*)d_mz2[m];
  p.e1 = (const Fr*)d_e1, p.e2 = (const Fr*)d_e2, p.t = (Fr*)d_t;
  k_nova_cross_term(ctx->c, p, *(const Fr*)u1, *(const Fr*)u2, (size_t)1 << dim_vars, out_bad);
  LH_CATCH
}
lh_status lh_debug_nova_fold(lh_ctx* ctx, size_t dim_vars, const lh_fr* d_w1, const lh_fr* d_w2, lh_fr* d_w_out, const lh_fr* d_e1,
                             const lh_fr* d_t, const lh_fr* d_e2, lh_fr* d_e_out, const lh_fr* r) {
  LH_TRY NEED_CTX(ctx);
  NEED(r);
  LH_REQUIRE(dim_vars >= 1 && dim_vars <= (size_t)LH_SPARTAN_MAX_DIM_VARS, LH_ERR_ARG, "nova: dim_vars out of range");
  HFr hr, hr2;
  memcpy(&hr, r, 32);
  hr2 = hr * hr;
  k_nova_fold(ctx->c, (const Fr*)d_w1, (const Fr*)d_w2, (Fr*)d_w_out, (const Fr*)d_e1, (const Fr*)d_t, (const Fr*)d_e2, (Fr*)d_e_out,
              *(const Fr*)&hr, *(const Fr*)&hr2, (size_t)1 << (dim_vars - 1), (size_t)1 << dim_vars);
  ctx->c.sync();
  LH_CATCH
}
lh_status lh_debug_sort_plan(size_t n, unsigned bits, int key_bytes, unsigned* passes, unsigned rb[8], size_t* temp_bytes) {
  LH_TRY
  NEED(passes);
  NEED(rb);
  NEED(temp_bytes);
  LH_REQUIRE(key_bytes == 4 || key_bytes == 8, LH_ERR_ARG, "debug sort: key_bytes is 4 or 8");
  sort_plan(n, bits, (size_t)key_bytes, passes, rb, temp_bytes);
  LH_CATCH
}
lh_status lh_debug_msm_plan(size_t num_jobs, const size_t* n, const uint32_t* bits, const uint32_t* kinds, int helper, int via_prepare,
                            uint64_t* out, size_t* num_subs) {
  LH_TRY
  NEED(n);
  NEED(bits);
  NEED(kinds);
  NEED(out);
  NEED(num_subs);
  LH_REQUIRE(num_jobs >= 1 && num_jobs <= 48, LH_ERR_ARG, "debug msm plan: 1 .. 48 jobs");
  Ctx c;  // (options and knobs as a ctx of this process would have them; no device behind it, and the plan asks for none)
  c.is_helper = helper != 0;
  std::vector<MsmJob> jobs;
  G1Affine second;
  for (size_t j = 0; j < num_jobs; j++) {
    LH_REQUIRE(bits[j] >= 1 && bits[j] <= (kinds[j] ? 32u : 254u), LH_ERR_ARG, "debug msm plan: bad width");
    MsmJob jb{nullptr, kinds[j] != 0, nullptr, n[j]};
    jb.known_bits = bits[j];
    if (kinds[j] >= 4) jb.pack_shift = kinds[j], jb.out_second = &second;
    jobs.push_back(jb);
  }
  *num_subs = msm_plan_shape(c, jobs.data(), num_jobs, via_prepare != 0, out);
  LH_CATCH
}
lh_status lh_debug_live_resources(uint64_t out[4]) {
  LH_TRY
  NEED(out);
  owned_live(out);
  LH_CATCH
}
lh_status lh_debug_fail_acquire_after(int64_t n) {
  LH_TRY
  owned_fail_acquire_after(n);
  LH_CATCH
}

// (development) the 32-bit column kernels (kernels_poly.hip, "small-valued columns") one launch set at a time:
// tests/test_gpu_u32_columns.py.  Everything is checked before anything is launched.
lh_status lh_debug_u32_columns(lh_ctx* ctx, int op, const lh_debug_u32_args* a) {
  LH_TRY NEED_CTX(ctx);
  NEED(a);
  Ctx& c = ctx->c;
  LH_REQUIRE((op >= LH_U32_INNER_PRODUCTS_SMALL && op <= LH_U32_SC_ROUND_BIND2) || op == LH_U32_QUAD_SUMS, LH_ERR_ARG,
             "debug u32 columns: unknown operation");
  LH_REQUIRE(a->n >= 1 && a->n < ((size_t)1 << 31), LH_ERR_ARG, "debug u32 columns: n must be in [1, 2^31)");
  const bool one_col = op == LH_U32_INNER_PRODUCTS_SMALL_QUADS || op == LH_U32_SC_ROUND_BIND2;
  const bool has_lens = op == LH_U32_INNER_PRODUCTS_QUADS || op == LH_U32_QUAD_SUMS || op == LH_U32_LINCOMB_MIXED ||
                        op == LH_U32_LINCOMB_FOLD_SMALL || op == LH_U32_LINCOMB_BIND2;
  const bool has_w = op == LH_U32_LINCOMB_MIXED || op == LH_U32_LINCOMB_FOLD_SMALL || op == LH_U32_LINCOMB_BIND2;
  const bool quads = op == LH_U32_INNER_PRODUCTS_SMALL_QUADS || op == LH_U32_INNER_PRODUCTS_QUADS || op == LH_U32_QUAD_SUMS ||
                     op == LH_U32_LINCOMB_BIND2 || op == LH_U32_SC_ROUND_BIND2;  // (the kernels that read a column as uint4)
  const bool sums = op != LH_U32_INNER_PRODUCTS_QUADS && op != LH_U32_QUAD_SUMS && op != LH_U32_LINCOMB_MIXED &&
                    op != LH_U32_LINCOMB_FOLD_SMALL;
  LH_REQUIRE(!one_col || a->count == 1, LH_ERR_ARG, "debug u32 columns: this operation takes one column");
  if (op == LH_U32_LINCOMB_MIXED)
    LH_REQUIRE(a->num_fr <= (size_t)LCM_MAX_FR && a->count <= (size_t)LCM_MAX_SMALL, LH_ERR_ARG, "debug u32 columns: too many inputs");
  else if (op == LH_U32_LINCOMB_BIND2)
    LH_REQUIRE(a->count >= 1 && a->count <= (size_t)LCB_MAX, LH_ERR_ARG, "debug u32 columns: bad column count");
  else
    LH_REQUIRE(a->count <= 1024, LH_ERR_ARG, "debug u32 columns: bad column count");
  NEED_N(a->d_cols, a->count);
  if (has_lens) NEED_N(a->lens, a->count);
  if (has_w) NEED_N(a->w, a->count);
  for (size_t k = 0; k < a->count; k++) {
    LH_REQUIRE(a->d_cols[k] != nullptr, LH_ERR_ARG, "null argument: a column");
    if (quads) {
      LH_REQUIRE((uintptr_t)a->d_cols[k] % 16 == 0, LH_ERR_ARG, "debug u32 columns: a column read as uint4 must be 16-byte aligned");
      LH_REQUIRE(!has_lens || a->lens[k] % 4 == 0, LH_ERR_ARG, "debug u32 columns: a column read as uint4 must have a multiple of 4 entries");
    }
  }
  if (op != LH_U32_LINCOMB_MIXED && op != LH_U32_LINCOMB_FOLD_SMALL) NEED(a->d_weights);
  if (op == LH_U32_LINCOMB_MIXED) {
    NEED_N(a->d_fr, a->num_fr);
    NEED_N(a->w_fr, a->num_fr);
    for (size_t k = 0; k < a->num_fr; k++) LH_REQUIRE(a->d_fr[k] != nullptr, LH_ERR_ARG, "null argument: a field-element table");
  }
  if (op == LH_U32_LINCOMB_FOLD_SMALL) NEED(a->taken);
  if (sums) NEED_N(a->out_host, op == LH_U32_INNER_PRODUCTS_SMALL || op == LH_U32_INNER_PRODUCTS_SMALL_HALF ? a->count : 1);
  if (op >= LH_U32_INNER_PRODUCTS_QUADS) NEED(a->d_out);
  const uint32_t* const* cols = a->d_cols;
  const Fr* dw = (const Fr*)a->d_weights;
  Fr r0, r1;
  memcpy(&r0, &a->r0, 32);
  memcpy(&r1, &a->r1, 32);
  ArenaScope scope(c.arena);  // (k_inner_products_quads leaves its partial sums to the caller's scope)
  switch (op) {
    case LH_U32_INNER_PRODUCTS_SMALL: k_inner_products_small(c, cols, a->count, dw, a->n, (Fr*)a->out_host); break;
    case LH_U32_INNER_PRODUCTS_SMALL_HALF: k_inner_products_small_half(c, cols, a->count, dw, a->n, r0, (Fr*)a->out_host); break;
    case LH_U32_INNER_PRODUCTS_SMALL_QUADS: k_inner_products_small_quads(c, cols[0], dw, a->n, (Fr*)a->out_host); break;
    case LH_U32_INNER_PRODUCTS_QUADS: k_inner_products_quads(c, cols, a->lens, a->count, dw, a->n, (Fr*)a->d_out); break;
    case LH_U32_QUAD_SUMS: k_quad_sums(c, cols, a->lens, a->count, dw, a->n, (Fr*)a->d_out); break;
    case LH_U32_LINCOMB_MIXED:
      k_lincomb_mixed(c, (const Fr* const*)a->d_fr, (const Fr*)a->w_fr, a->num_fr, cols, a->lens, (const Fr*)a->w, a->count, a->n,
                      (Fr*)a->d_out);
      break;
    case LH_U32_LINCOMB_FOLD_SMALL:  // (false - no columns, too many, nothing to fold - is the caller's cue for the other route)
      *a->taken = k_lincomb_fold_small(c, cols, a->lens, (const Fr*)a->w, a->count, a->n, r0, (Fr*)a->d_out) ? 1 : 0;
      break;
    default: {
      // the round sums land in pinned memory of the ctx, behind the argument block of k_lincomb_bind2 (as sumcheck.cpp does)
      Fr* two = (Fr*)c.pin(65536) + 1024;
      if (op == LH_U32_LINCOMB_BIND2) {
        k_lincomb_bind2(c, cols, a->lens, (const Fr*)a->w, a->count, r0, r1, dw, a->n, (Fr*)a->d_out, two);
        memcpy(a->out_host, two, 64);
      } else {
        k_sc_round_u32_bind2(c, cols[0], dw, r0, r1, a->n, (Fr*)a->d_out, two);
        memcpy(a->out_host, two, 32);
      }
    }
  }
  c.sync();
  LH_CATCH
}

// (development) the witness step's subtable read for one memory: tests/test_gpu_lasso_custom.py
lh_status lh_debug_lasso_subtable_read(lh_ctx* ctx, uint32_t kind, uint32_t chunk_bits, const uint32_t* d_dim, size_t n,
                                       uint32_t* d_out) {
  LH_TRY NEED_CTX(ctx);
  NEED(d_dim);
  NEED(d_out);
  Ctx& c = ctx->c;
  LH_REQUIRE(n >= 1 && n < ((size_t)1 << 31), LH_ERR_ARG, "debug subtable read: n must be in [1, 2^31)");
  LH_REQUIRE(chunk_bits >= 1 && chunk_bits < 31, LH_ERR_ARG, "lasso: need at least one variable");
  if (subtable_is_custom(kind)) {
    subtable_require(kind, chunk_bits);
  } else {
    LH_REQUIRE(kind < LH_SUBTABLE_KINDS, LH_ERR_ARG, "lasso: unknown subtable");
    if (kind != LH_SUBTABLE_IDENTITY)
      LH_REQUIRE(chunk_bits % 2 == 0, LH_ERR_ARG, "lasso: bitwise subtables need an even chunk_bits");
  }
  ArenaScope scope(c.arena);
  SubtableOrders tables(c, chunk_bits);  // (its staging outlives the sync below)
  if (kind == LH_SUBTABLE_IDENTITY)
    LH_HIP(hipMemcpyAsync(d_out, d_dim, n * 4, hipMemcpyDeviceToDevice, c.stream));  // (the witness step shares the column)
  else
    k_lasso_subtable_read(c, (int)kind, chunk_bits, d_dim, n, d_out, subtable_is_custom(kind) ? tables.custom_table(kind) : nullptr);
  c.sync();
  LH_CATCH
}

lh_status lh_profile_enable(lh_ctx* ctx, int on) {
  LH_TRY NEED_CTX(ctx);
  ctx->c.sync();
  ctx->c.prof = on == 1;
  ctx->c.prof_recs.clear();
  // 2: live records of the bucket-accumulation launches only (dev.hpp Ctx::live); the helper ctx's launches count too
  std::vector<ProfRec> drop;
  ctx->c.live_resolve(drop);
  ctx->c.live = on == 2;
  if (ctx->c.helper) {
    ctx->c.helper->live_resolve(drop);
    ctx->c.helper->live = on == 2;
  }
  LH_CATCH
}
lh_status lh_profile_read(lh_ctx* ctx, lh_prof_rec* out, size_t cap, size_t* count) {
  LH_TRY NEED_CTX(ctx);
  NEED(count);
  static_assert(sizeof(lh_prof_rec) == sizeof(lh::ProfRec), "profile record layout");
  if (ctx->c.live) {  // (resolved at the first read after the timed region: waits for the streams)
    ctx->c.live_resolve(ctx->c.prof_recs);
    if (ctx->c.helper) {
      LH_HIP(hipStreamSynchronize(ctx->c.helper->stream));
      ctx->c.helper->live_resolve(ctx->c.prof_recs);
    }
  }
  size_t n = ctx->c.prof_recs.size();
  *count = n;
  if (out && cap) memcpy(out, ctx->c.prof_recs.data(), (n < cap ? n : cap) * sizeof(lh_prof_rec));
  LH_CATCH
}

}  // extern "C"
