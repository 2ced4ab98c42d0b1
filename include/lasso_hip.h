/* lasso_hip.h -- C-ABI of the MI355X-native prover hot path (liblasso_hip.so).
 *
 * The reference (DoHoonKim8/halo2-lasso, Rust) has no FFI: its seam is a set of generic traits
 * (SURVEY.md §8b).  Every entry point below names the reference item it replaces; a Rust shim
 * implementing those traits binds exactly these symbols.
 *
 * Conventions
 *  - Field elements cross the ABI in halo2curves' in-memory form: 4 x u64 little-endian limbs,
 *    Montgomery (R = 2^256).  `lh_fr` is therefore bit-identical to a Rust `bn256::Fr`, and
 *    `lh_g1` ({x, y} in Fq, identity = (0,0)) to `bn256::G1Affine`.
 *  - `d_*` arguments are DEVICE pointers (from lh_alloc, or any HIP allocation such as a torch
 *    tensor's data_ptr on the ctx's device); everything else is host memory owned by the caller
 *    for the duration of the call.
 *  - Every function returns an `lh_status`; 0 is success, negatives mirror
 *    plonkish_backend::Error (plonkish_backend/src/lib.rs:12-20).  lh_last_error() gives the
 *    message of the last failure on the calling thread.
 *  - One ctx per process per GPU; calls on one ctx are not re-entrant (the reference calls
 *    `prove` from one thread and fans out on rayon, util/parallel.rs:9-46).  A ctx may start host threads of its own and a
 *    helper ctx on the same device (second stream, own arena and pinned blocks: lh_lasso_prove commits the challenge-free
 *    part of its opening there, option open_precommit); both end with the call that started them / with lh_ctx_destroy.
 *  - There is NO CPU fallback: without a usable HIP device lh_ctx_create fails with
 *    LH_ERR_DEVICE and nothing else can be called.
 *  - Every entry point that takes an lh_ctx makes the ctx's HIP device current for the duration of the
 *    call (and restores the caller's): a ctx may be used from any host thread, one call at a time.
 *  - The last rounds of a sum-check run inside ONE resident kernel that exchanges message and challenge
 *    with the calling thread through pinned memory while the lh_* call is in progress.  The kernel waits a
 *    bounded time for each challenge (environment LH_SC_TAIL_TIMEOUT_MS, default 2000); when the calling
 *    thread stalls longer (debugger, SIGSTOP, slow transcript callback) the prover resumes with launched
 *    rounds - same proof bytes, no error.  LH_SC_TAIL=0 disables the resident rounds.  (The kernel is at most 64
 *    workgroups that wait for the host only, never for one another or for another kernel; messages and challenges
 *    cross as 16-byte chunks that carry their own sequence number, written with single 16-byte stores: the host
 *    side is x86-64 with SSE2.)
 */
#ifndef LASSO_HIP_H
#define LASSO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct { uint64_t l[4]; } lh_fr;      /* bn256::Fr, Montgomery */
typedef struct { uint64_t x[4], y[4]; } lh_g1; /* bn256::G1Affine, Montgomery Fq coords */

typedef int lh_status;
#define LH_OK 0
#define LH_ERR_INVALID_SUMCHECK (-1)  /* Error::InvalidSumcheck  lib.rs:14 */
#define LH_ERR_INVALID_PCS_PARAM (-2) /* Error::InvalidPcsParam  lib.rs:15 */
#define LH_ERR_INVALID_PCS_OPEN (-3)  /* Error::InvalidPcsOpen   lib.rs:16 */
#define LH_ERR_INVALID_SNARK (-4)     /* Error::InvalidSnark     lib.rs:17 */
#define LH_ERR_SERIALIZATION (-5)     /* Error::Serialization    lib.rs:18 */
#define LH_ERR_TRANSCRIPT (-6)        /* Error::Transcript       lib.rs:19 */
#define LH_ERR_DEVICE (-7)            /* no HIP device / HIP runtime failure */
#define LH_ERR_ARG (-8)               /* assert!/panic in the reference: bad argument */

typedef struct lh_ctx lh_ctx;

const char* lh_last_error(void);
const char* lh_version(void);

/* ---------------------------------------------------------------- context & memory */
lh_status lh_ctx_create(int device_id, lh_ctx** out);
void lh_ctx_destroy(lh_ctx* ctx);
lh_status lh_ctx_sync(lh_ctx* ctx);
/* opaque hipStream_t the ctx launches on (for bench.py's HIP-event timing) */
void* lh_ctx_stream(lh_ctx* ctx);
lh_status lh_alloc(lh_ctx* ctx, size_t bytes, void** d_out);
lh_status lh_free(lh_ctx* ctx, void* d_ptr);
lh_status lh_upload(lh_ctx* ctx, void* d_dst, const void* src, size_t bytes);
lh_status lh_download(lh_ctx* ctx, void* dst, const void* d_src, size_t bytes);

/* ---------------------------------------------------------------- transcript
 * Callback table standing for `&mut impl TranscriptWrite<G1Affine, Fr>`
 * (util/transcript.rs:15-97).  Each callback returns 0 or a negative lh_status. */
typedef struct lh_transcript {
  void* user;
  int (*write_field_element)(void* user, const lh_fr* fe);  /* transcript.rs:157-165 */
  int (*common_field_element)(void* user, const lh_fr* fe); /* transcript.rs:133-136 */
  int (*squeeze_challenge)(void* user, lh_fr* out);          /* transcript.rs:126-131 */
  int (*write_commitment)(void* user, const lh_g1* pt);     /* transcript.rs:213-226 */
  int (*common_commitment)(void* user, const lh_g1* pt);    /* transcript.rs:170-183 */
  /* TranscriptRead half (verifiers only; may be NULL on a write-only transcript) */
  int (*read_field_element)(void* user, lh_fr* out);         /* transcript.rs:138-154 */
  int (*read_commitment)(void* user, lh_g1* out);            /* transcript.rs:185-210 */
} lh_transcript;

/* Built-in Keccak256Transcript<Cursor<Vec<u8>>> (transcript.rs:99-121) */
lh_status lh_keccak_transcript_new(lh_transcript** out);
void lh_keccak_transcript_free(lh_transcript* t);
/* InMemoryTranscript::into_proof (transcript.rs:110-112): pointer valid until the next write */
lh_status lh_keccak_transcript_proof(lh_transcript* t, const uint8_t** bytes, size_t* len);
/* InMemoryTranscript::from_proof (transcript.rs:114-123): a reading transcript over a copy of `proof` */
lh_status lh_keccak_transcript_from_proof(const uint8_t* proof, size_t len, lh_transcript** out);
/* bytes of the proof not yet read */
lh_status lh_keccak_transcript_remaining(lh_transcript* t, size_t* out);

/* ---------------------------------------------------------------- a1: Fr arithmetic
 * halo2_curves bn256::Fr ops (via util/arithmetic.rs:15-22) over device vectors. */
lh_status lh_fr_from_u64(lh_ctx*, const uint64_t* d_in, size_t n, lh_fr* d_out); /* Fr::from(u64) */
lh_status lh_fr_from_u32(lh_ctx*, const uint32_t* d_in, size_t n, lh_fr* d_out);
lh_status lh_fr_to_repr(lh_ctx*, const lh_fr* d_in, size_t n, uint8_t* d_out32); /* to_repr(): canonical LE */
lh_status lh_fr_from_repr(lh_ctx*, const uint8_t* d_in32, size_t n, lh_fr* d_out); /* must be < r */
lh_status lh_fr_add(lh_ctx*, const lh_fr* d_a, const lh_fr* d_b, size_t n, lh_fr* d_out);
lh_status lh_fr_sub(lh_ctx*, const lh_fr* d_a, const lh_fr* d_b, size_t n, lh_fr* d_out);
lh_status lh_fr_mul(lh_ctx*, const lh_fr* d_a, const lh_fr* d_b, size_t n, lh_fr* d_out);
/* `iters` dependent multiplications per element: peak Fr-mul/s micro-benchmark */
lh_status lh_fr_mul_chain(lh_ctx*, const lh_fr* d_a, const lh_fr* d_b, size_t n, int iters, lh_fr* d_out);
/* ff::BatchInvert (call sites prover.rs:226-234, arithmetic.rs:121): zeros stay zero */
lh_status lh_fr_batch_invert(lh_ctx*, const lh_fr* d_in, size_t n, lh_fr* d_out);

/* ---------------------------------------------------------------- a3/a4: MultilinearPolynomial
 * poly/multilinear.rs.  Tables are 2^num_vars device lh_fr, index bit i <-> variable i. */
/* fix_var (multilinear.rs:179-183,599-618): d_out[b] = e[2b] + (e[2b+1]-e[2b])*x, n_in = 2^m */
lh_status lh_fix_var(lh_ctx*, const lh_fr* d_in, size_t n_in, const lh_fr* x, lh_fr* d_out);
/* eq_xy (multilinear.rs:91-127): d_out has 2^num_vars entries */
lh_status lh_eq_xy(lh_ctx*, const lh_fr* y, size_t num_vars, lh_fr* d_out);
/* evaluate (multilinear.rs:137-156) of `num_polys` tables at one point */
lh_status lh_evaluate(lh_ctx*, const lh_fr* const* d_polys, size_t num_polys, size_t num_vars,
                      const lh_fr* point, lh_fr* out_evals);
/* AddAssign<(&F,&Self)> folded (multilinear.rs:294-320): d_out = sum_i w[i] * d_polys[i] */
lh_status lh_lincomb(lh_ctx*, const lh_fr* const* d_polys, const lh_fr* w, size_t num_polys,
                     size_t n, lh_fr* d_out);

/* ---------------------------------------------------------------- a5-a8: piop::sum_check
 * ClassicSumCheck::prove (piop/sum_check/classic.rs:208-240) for expressions of the form
 *     [eq_xy(ys[eq_y]) *]  sum_m coeff[m] * prod_k table[factor[m][k]]
 * which covers fractional_sum_check.rs:272-281, pcs/multilinear.rs:182-190 and the Surge /
 * grand-product expressions.  Table ids < num_polys name d_polys, ids >= num_polys name
 * eq_xy(ys[id - num_polys]).  `degree` is Expression::degree() (expression.rs:171-182). */
#define LH_SC_MAX_TERMS 48
#define LH_SC_MAX_FACTORS 4
typedef struct lh_sop {
  uint32_t num_terms;
  int32_t global_eq; /* index into ys multiplied onto the whole sum, or -1 */
  lh_fr coeff[LH_SC_MAX_TERMS];
  uint8_t num_factors[LH_SC_MAX_TERMS];
  uint8_t factor[LH_SC_MAX_TERMS][LH_SC_MAX_FACTORS];
} lh_sop;

#define LH_SC_EVALUATIONS 0  /* EvaluationsProver  classic/eval.rs:68-131: d+1 evals per round */
#define LH_SC_COEFFICIENTS 1 /* CoefficientsProver classic/coeff.rs:62-150: 3 coeffs, degree 2 */
/* Returns challenges x (num_vars) and evals = each poly at x (classic.rs:143-149). */
lh_status lh_sumcheck_prove(lh_ctx*, int prover_kind, size_t num_vars, const lh_sop* expr,
                            const lh_fr* const* d_polys, size_t num_polys,
                            const lh_fr* ys, size_t num_ys, /* num_ys points of num_vars each */
                            const lh_fr* sum, lh_transcript* t,
                            lh_fr* out_challenges, lh_fr* out_evals);

/* General Expression (util/expression.rs:67-78), flattened: every node refers to EARLIER nodes, the
 * root is the last one.  DistributePowers(exprs, base) is lowered by the caller exactly as
 * Expression::evaluate does (expression.rs:155-167): e0 + base*e1 + base^2*e2 + ...            */
#define LH_EX_CONSTANT 0   /* scalar */
#define LH_EX_IDENTITY 1   /* CommonPolynomial::Identity */
#define LH_EX_LAGRANGE 2   /* CommonPolynomial::Lagrange(a) */
#define LH_EX_EQ_XY 3      /* CommonPolynomial::EqXY(a) */
#define LH_EX_POLYNOMIAL 4 /* Query { poly: a, rotation: b } */
#define LH_EX_CHALLENGE 5  /* Challenge(a) */
#define LH_EX_NEGATED 6    /* -node[a] */
#define LH_EX_SUM 7        /* node[a] + node[b] */
#define LH_EX_PRODUCT 8    /* node[a] * node[b] */
#define LH_EX_SCALED 9     /* node[a] * scalar */
typedef struct lh_expr_node { uint32_t op; int32_t a, b; uint32_t reserved; lh_fr scalar; } lh_expr_node;
typedef struct lh_expr { const lh_expr_node* nodes; size_t num_nodes; } lh_expr;
/* ClassicSumCheck::<EvaluationsProver>::prove over a VirtualPolynomial{expression, polys, challenges, ys}
 * (piop/sum_check.rs:16-37, classic.rs:208-240) including rotations (BooleanHypercube, util/arithmetic/bh.rs),
 * Identity and Lagrange.  out_evals: every poly at x (classic.rs:143-149). */
lh_status lh_sumcheck_prove_expr(lh_ctx*, size_t num_vars, const lh_expr* expr, const lh_fr* const* d_polys,
                                 size_t num_polys, const lh_fr* challenges, size_t num_challenges,
                                 const lh_fr* ys, size_t num_ys, const lh_fr* sum, lh_transcript* t,
                                 lh_fr* out_challenges, lh_fr* out_evals);

/* ---------------------------------------------------------------- a9: piop::gkr
 * prove_fractional_sum_check (piop/gkr/fractional_sum_check.rs:89-190).  claimed_*[b] may be
 * NULL (None => root written) or point to a claim (Some => root only hashed).  Outputs
 * p_xs[B], q_xs[B], x[num_vars]. */
lh_status lh_gkr_fractional_prove(lh_ctx*, size_t num_batching, size_t num_vars,
                                  const lh_fr* const* claimed_p_0s, const lh_fr* const* claimed_q_0s,
                                  const lh_fr* const* d_ps, const lh_fr* const* d_qs,
                                  lh_transcript* t, lh_fr* out_p_xs, lh_fr* out_q_xs, lh_fr* out_x);
/* Product-only layered circuit used by the Lasso memory check (no reference code; layering
 * and schedule follow fractional_sum_check.rs:62-190 with p dropped).  Trees may have different
 * depth (num_vars[b] >= 1).  out_points holds, per tree, num_vars[b] elements back to back. */
lh_status lh_grand_product_prove(lh_ctx*, size_t num_trees, const lh_fr* const* d_leaves,
                                 const size_t* num_vars, lh_transcript* t, lh_fr* out_roots,
                                 lh_fr* out_claims, lh_fr* out_points);

/* ---------------------------------------------------------------- a10: util::arithmetic::msm
 * variable_base_msm (util/arithmetic/msm.rs:84-181); result normalised to affine. */
lh_status lh_msm(lh_ctx*, const lh_fr* d_scalars, const lh_g1* d_bases, size_t n, lh_g1* out);
/* same with u32 scalars (Lasso's dim / read_ts / final_cts / E polys are small-valued) */
lh_status lh_msm_u32(lh_ctx*, const uint32_t* d_scalars, const lh_g1* d_bases, size_t n, lh_g1* out);

/* ---------------------------------------------------------------- a11/a12: pcs::multilinear::kzg */
typedef struct lh_srs lh_srs; /* MultilinearKzgProverParams (kzg.rs:56-77): eqs[0..=num_vars] on device */
/* setup (kzg.rs:166-228) with the trapdoor given explicitly: eqs[k][b] = eq_k(b; s) * G */
lh_status lh_mkzg_setup(lh_ctx*, const lh_fr* ss, size_t num_vars, lh_srs** out);
/* upload of an existing param: eqs flattened, level k at offset 2^k - 1 (trim, kzg.rs:230-250) */
lh_status lh_srs_upload(lh_ctx*, const lh_g1* eqs_flat, size_t num_vars, lh_srs** out);
lh_status lh_srs_download(lh_ctx*, const lh_srs*, lh_g1* eqs_flat);
size_t lh_srs_num_vars(const lh_srs*);
void lh_srs_free(lh_ctx*, lh_srs*);
/* commit / batch_commit (kzg.rs:252-274) */
lh_status lh_mkzg_commit(lh_ctx*, const lh_srs*, const lh_fr* d_poly, size_t num_vars, lh_g1* out);
lh_status lh_mkzg_batch_commit(lh_ctx*, const lh_srs*, const lh_fr* const* d_polys, size_t num_polys,
                               size_t num_vars, lh_g1* out_comms);
/* open (kzg.rs:276-302): writes n quotient commitments to the transcript; *out_eval = remainder */
lh_status lh_mkzg_open(lh_ctx*, const lh_srs*, const lh_fr* d_poly, size_t num_vars,
                       const lh_fr* point, lh_transcript* t, lh_fr* out_eval);
/* batch_open (pcs/multilinear.rs:134-235); Evaluation = {poly, point, value} (pcs.rs:132-155) */
typedef struct lh_evaluation { uint32_t poly, point; lh_fr value; } lh_evaluation;
lh_status lh_mkzg_batch_open(lh_ctx*, const lh_srs*, size_t num_vars,
                             const lh_fr* const* d_polys, size_t num_polys,
                             const lh_fr* points, size_t num_points,
                             const lh_evaluation* evals, size_t num_evals, lh_transcript* t);

/* ---------------------------------------------------------------- a': Lasso lookup argument
 * No reference code (README.md:1-9 only); protocol specified in oracle/pyref/lasso.py. */
#define LH_SUBTABLE_IDENTITY 0
#define LH_SUBTABLE_AND 1
#define LH_SUBTABLE_XOR 2
/* Index m = x || y with y in the low chunk_bits / 2 bits, as for AND and XOR (an even chunk_bits, or LH_ERR_ARG):
 *   OR   T[m] = x | y        values of chunk_bits / 2 bits
 *   EQ   T[m] = (x == y)     one bit
 *   LTU  T[m] = (x <  y)     one bit, unsigned
 * Equality of two (c chunk_bits / 2)-bit operands is g = prod_j E_EQ_j, unsigned less-than is
 * g = sum_j E_LTU_j prod_{k > j} E_EQ_k (chunk 0 least significant): the longest term has c factors, so such a table has
 * c <= LH_SC_MAX_FACTORS chunks (a term with more factors is LH_ERR_ARG like any other bad g term). */
#define LH_SUBTABLE_OR 3
#define LH_SUBTABLE_EQ 4
#define LH_SUBTABLE_LTU 5
/* Caller-registered subtables: any table of 2^chunk_bits 32-bit entries the caller can write down (a signed comparison's
 * top chunk, a shift, an S-box, a popcount).  Lasso needs no formula for a subtable: the prover reads the entries, the
 * verifier evaluates their multilinear extension at one point (O(2^chunk_bits) host work).  The registry is process-wide,
 * thread-safe and needs no ctx (the verifier has none).
 *   lh_subtable_register   copies the 2^chunk_bits host values and returns a new kind, LH_SUBTABLE_CUSTOM_BASE + the number
 *                          of registrations made before it in this process: kinds are never reused, so a stale kind is
 *                          refused and never silently another table.  Kinds 6 .. 0xFF stay LH_ERR_ARG.
 *   lh_subtable_unregister forgets the kind; a prove or verify that has already looked the table up keeps its entries alive.
 *   lh_subtable_info       chunk_bits, value_bits (the bit length of the largest entry; 0 for an all-zero table) and the
 *                          Keccak-256 digest of the entries as little-endian 32-bit words (any of the three may be NULL).
 *                          The digest lets a prover and a verifier on different hosts compare what they registered.  It is
 *                          NOT absorbed into any transcript: the table is part of the statement, as the kinds are.
 * LH_ERR_ARG: a NULL `values` / `out_kind`, chunk_bits 0 or above LH_SUBTABLE_CUSTOM_MAX_BITS, more than
 * LH_SUBTABLE_CUSTOM_MAX live registrations, an unknown kind.
 * A memory of an lh_lasso_table may name a registered kind: the table's chunk_bits must equal the registered one
 * (LH_ERR_ARG otherwise; an odd chunk_bits is fine - the even rule belongs to the x || y kinds above).  Such a memory's
 * column E = T[dim] is committed from the buckets of dim's commitment when T[0] = 0 and as an ordinary 32-bit column
 * otherwise; every prover and every PCS that takes an lh_lasso_table takes it. */
#define LH_SUBTABLE_CUSTOM_BASE 0x100u
#define LH_SUBTABLE_CUSTOM_MAX 64
#define LH_SUBTABLE_CUSTOM_MAX_BITS 20
lh_status lh_subtable_register(const uint32_t* values /* host, 2^chunk_bits */, uint32_t chunk_bits, uint32_t* out_kind);
lh_status lh_subtable_unregister(uint32_t kind);
lh_status lh_subtable_info(uint32_t kind, uint32_t* chunk_bits, uint32_t* value_bits, uint8_t digest32[32]);
#define LH_LASSO_MAX_CHUNKS 8
#define LH_LASSO_MAX_MEMORIES 16
#define LH_LASSO_MAX_TERMS 16
typedef struct lh_lasso_table {
  uint32_t num_chunks;   /* c */
  uint32_t chunk_bits;   /* l : subtable size 2^l */
  uint32_t num_memories; /* alpha */
  uint32_t memory_chunk[LH_LASSO_MAX_MEMORIES];    /* j(i) */
  uint32_t memory_subtable[LH_LASSO_MAX_MEMORIES]; /* LH_SUBTABLE_*, or a kind of lh_subtable_register */
  uint32_t num_terms; /* g = sum_m coeff[m] * prod_{k < num_factors[m]} E_{factor[m][k]} */
  lh_fr g_coeff[LH_LASSO_MAX_TERMS];
  uint8_t g_num_factors[LH_LASSO_MAX_TERMS];
  uint8_t g_factor[LH_LASSO_MAX_TERMS][LH_SC_MAX_FACTORS];
} lh_lasso_table;
/* d_dims[j]: device u32[2^num_vars] chunk indices (< 2^chunk_bits) of every lookup. */
lh_status lh_lasso_prove(lh_ctx*, const lh_srs*, const lh_lasso_table*, size_t num_vars,
                         const uint32_t* const* d_dims, lh_transcript* t);

/* ---------------------------------------------------------------- a'': lookups into several tables in ONE proof
 * num_tables tables with the same number of lookups 2^num_vars, each with its own lh_lasso_table and its own chunk
 * columns (d_dims[t][j]: chunk column j of table t), argued over one transcript with one commit batch, one Surge
 * sum-check (eq * sum_t rho^t g_t), one grand-product GKR over all memories and one batch opening; multilinear KZG.  The
 * protocol is specified in tests/lasso_batch_ref.py; num_tables = 1 is not special-cased and its bytes
 * differ from lh_lasso_prove's.  Every poly is zero-padded to nv = max(num_vars, max_t chunk_bits_t) variables, so a
 * table's commitment block is the block of its own lh_lasso_prove proof whenever that proof's nv is the same.  Two tables
 * of equal chunk_bits that are handed the SAME device pointer for a chunk column (AND and XOR over the same operands) share
 * that column's counters, read_ts, final_cts and commitment jobs; the transcript still carries both blocks.
 * Limits (LH_ERR_ARG with a message, checked on entry):
 *   1 <= num_tables <= LH_LASSO_BATCH_MAX_TABLES; no NULL table, column or list; every table passes lh_lasso_prove's checks
 *   sum of num_memories <= 8     the batch has 4 * that many product trees, and one GKR layer takes 2 B + 1 <= 72 tables
 *   sum of num_terms <= LH_SC_MAX_TERMS   the Surge sum-check's terms
 *   1 + 3 num_chunks + num_memories <= 63 per table   one identity mask per table
 *   sum of 2 num_chunks + num_memories <= 24   the columns the batch opening merges at one point in one launch
 *   not on a ctx inside a sharded prove, nor on one with a communicator of more than one rank attached
 * LH_ERR_INVALID_PCS_PARAM when nv exceeds the SRS.  lh_lasso_last_timing and lh_lasso_last_route report a batch prove
 * like a single one.  The verifier is host only. */
#define LH_LASSO_BATCH_MAX_TABLES 8
lh_status lh_lasso_prove_batch(lh_ctx*, const lh_srs*, const lh_lasso_table* const* tables, size_t num_tables, size_t num_vars,
                               const uint32_t* const* const* d_dims, lh_transcript* t);
/* (lh_lasso_verify_batch: with the verifiers below) */

/* ---------------------------------------------------------------- a''': LogUp-GKR, a lookup argument for unstructured tables
 * Lasso serves tables that decompose into subtables read by index.  This argument serves the others: a table whose rows
 * are arbitrary field elements, or tuples of them, looked up BY VALUE (a ROM of constants, an opcode / operand / result
 * relation, a round-constant schedule).  It proves the LogUp identity
 *     sum_i 1 / (gamma + f[i])  =  sum_r m[r] / (gamma + t[r])
 * with two fractional sum-checks (piop/gkr/fractional_sum_check.rs, the paper it cites) and commits only the inputs and the
 * small-valued multiplicities m - no helper column.  The protocol is specified in tests/logup_gkr_ref.py.
 *
 * num_lookups lookups share num_vars (2^num_vars input rows each) and table_vars (2^table_vars table rows each; a shorter
 * table is padded by repeating a row - duplicates are legal, the LAST of equal rows takes every count).  Lookup k:
 *   width     w_k columns: a row is a tuple of w_k field elements, compressed as sum_j beta^j column_j
 *   d_inputs  w_k DEVICE columns of 2^num_vars Montgomery lh_fr; the verifier ignores them: NULL allowed there
 *   table     w_k HOST columns of 2^table_vars Montgomery lh_fr, the same values for prover and verifier
 * The table is part of the statement, like the entries of a registered subtable: it is NOT absorbed into the transcript.
 * Every committed poly is zero-padded to nv = max(num_vars, table_vars) variables.
 * Limits (LH_ERR_ARG with a message, checked on entry):
 *   1 <= num_lookups <= LH_LOGUP_MAX_LOOKUPS, 1 <= width <= LH_LOGUP_MAX_WIDTH   one launch per side, columns in the arguments
 *   sum of widths <= 63                    one identity mask frames the input commitments (another the multiplicities')
 *   1 <= num_vars < 31, 1 <= table_vars <= LH_LOGUP_MAX_TABLE_VARS   the verifier's table evaluation is linear in the table
 *   no NULL lookup, column or list; not on a ctx inside a sharded prove, nor on one with a communicator of several ranks
 * LH_ERR_INVALID_PCS_PARAM when nv exceeds the SRS; LH_ERR_INVALID_SNARK "Invalid lookup input" when an input row is in
 * no table row (the ctx stays usable).  Route option logup_fused_leaves below. */
#define LH_LOGUP_MAX_LOOKUPS 8
#define LH_LOGUP_MAX_WIDTH 8
#define LH_LOGUP_MAX_TABLE_VARS 24
typedef struct lh_logup_lookup {
  uint32_t width;
  const lh_fr* const* d_inputs; /* device */
  const lh_fr* const* table;    /* host */
} lh_logup_lookup;
lh_status lh_logup_gkr_prove(lh_ctx*, const lh_srs*, const lh_logup_lookup* lookups, size_t num_lookups, size_t num_vars,
                             size_t table_vars, lh_transcript* t);
/* The same proof from input columns of which some (or all) are 32-bit words: column j of a lookup has the type kinds[j]
 * says.  A u32 column and the same values as lh_fr are the same polynomial: the proof bytes are those of lh_logup_gkr_prove on
 * the widened columns and are verified by lh_logup_gkr_verify with the plain lh_logup_lookup list (no verifier entry of its
 * own).  A u32 column is committed as a 32-bit MSM over its 2^num_vars entries, compressed by 8 multiply-adds per entry,
 * evaluated and opened as a small column - never widened, never padded.  Limits and errors as above; a kind
 * other than the two below is LH_ERR_ARG with a message naming the lookup and the column. */
#define LH_LOGUP_COL_FR  0   /* lh_fr[2^num_vars], Montgomery */
#define LH_LOGUP_COL_U32 1   /* uint32_t[2^num_vars], any 32-bit value */
typedef struct lh_logup_columns {
  uint32_t width;
  const void* const* d_inputs;   /* device; column j has the type kinds[j] says */
  const uint8_t* kinds;          /* width entries; NULL = all LH_LOGUP_COL_FR */
  const lh_fr* const* table;     /* host, as in lh_logup_lookup */
} lh_logup_columns;
lh_status lh_logup_gkr_prove_columns(lh_ctx*, const lh_srs*, const lh_logup_columns* lookups, size_t num_lookups,
                                     size_t num_vars, size_t table_vars, lh_transcript* t);
/* (lh_logup_gkr_verify, lh_gkr_fractional_verify: with the verifiers below) */

/* ---------------------------------------------------------------- a'''': read-write memory checking, an argument for RAM traces
 * Lasso and LogUp-GKR check memories that never change.  This argument checks one that does: a memory of 2^mem_vars cells of
 * 32-bit words and a trace of 2^num_vars operations, three DEVICE columns of uint32_t[2^num_vars].  Operation i says that cell
 * d_addr[i] held d_rv[i] before it and holds d_wv[i] after it (a load: wv = rv).  Proven: every address is below 2^mem_vars,
 * and every rv[i] is the wv of the latest earlier operation on the same cell, or init[addr[i]] when there is none.  Operation i
 * writes at time i + 1, the image has time 0; no timestamp is handed in.  The protocol is specified in tests/memcheck_ref.py
 * (DESIGN.md §21): offline memory checking (Init u WS = RS u Final as multisets, one grand-product GKR over four trees) plus
 * a LogUp range check of the differences i - rt[i] in [0, 2^num_vars) (one fractional sum-check over two fractions) - without
 * the latter a read from the future would pass.
 *
 * init is HOST memory, 2^mem_vars words, or NULL for an all-zero image.  It is part of the statement, like a LogUp-GKR table:
 * it is NOT absorbed into the transcript; init given and NULL are different statements even when every word is zero.
 * The proof commits seven 32-bit columns - addr, rv, wv, the previous-write times rt, the final values fv and times ft, the
 * multiplicities m of the differences - each over its own length against the bases of nv = max(num_vars, mem_vars) variables,
 * in ONE block framed by an identity mask.  The first three commitments of the proof are addr, rv, wv at nv variables: what a
 * caller links to another proof about the same columns.
 * Limits (LH_ERR_ARG with a message, checked on entry):
 *   1 <= num_vars < 31                       positions and times are 32-bit words
 *   1 <= mem_vars <= LH_MEMCHECK_MAX_INIT_VARS with an image   the verifier folds the 2^mem_vars words of the image
 *   1 <= mem_vars < 31 without one           addresses are 32-bit words
 *   no NULL trace or column; not on a ctx inside a sharded prove, nor on one with a communicator of several ranks
 * LH_ERR_INVALID_PCS_PARAM when nv exceeds the SRS; LH_ERR_INVALID_SNARK "Invalid memory trace" when the trace is not
 * consistent or an address is out of range (the ctx stays usable).  Multilinear KZG only.  Route option logup_fused_leaves
 * below covers the leaf kernels of this argument too. */
#define LH_MEMCHECK_MAX_INIT_VARS 24
typedef struct lh_memcheck_trace {
  const uint32_t *d_addr, *d_rv, *d_wv; /* device, 2^num_vars each */
} lh_memcheck_trace;
lh_status lh_memcheck_prove(lh_ctx*, const lh_srs*, const lh_memcheck_trace*, size_t num_vars, size_t mem_vars,
                            const uint32_t* init /* host, 2^mem_vars, or NULL */, lh_transcript* t);
/* (lh_memcheck_verify: with the verifiers below; lh_debug_memcheck_witness: with the debug entries) */

/* The trace from the operations, on the device.  A front end knows (address, load or store, stored word) per
 * operation: operation i is a store of d_val[i] when d_store[i] != 0, otherwise a load (d_val[i] is ignored).  Written:
 *   d_rv[i]    the word stored by the latest earlier store to d_addr[i], or d_image[d_addr[i]] when there is none
 *   d_wv[i]    d_store[i] ? d_val[i] : d_rv[i]
 *   d_final[a] the word of cell a after the trace (NULL: not wanted)
 * (d_addr, d_rv, d_wv) is then the trace lh_memcheck_prove and lh_memcheck_prove_segment take.  d_image is DEVICE memory,
 * 2^mem_vars words, or NULL for an all-zero image.  Limits: 1 <= num_vars < 31, 1 <= mem_vars < 31, no NULL column
 * (LH_ERR_ARG).  An address >= 2^mem_vars: LH_ERR_INVALID_SNARK "Invalid memory trace" (one flag readback; the outputs are
 * then unspecified, the ctx stays usable).  Nothing else can be invalid. */
typedef struct lh_memcheck_ops {
  const uint32_t *d_addr, *d_store, *d_val; /* device, 2^num_vars each */
} lh_memcheck_ops;
lh_status lh_memcheck_replay(lh_ctx*, const lh_memcheck_ops*, size_t num_vars, size_t mem_vars,
                             const uint32_t* d_image /* device, 2^mem_vars, or NULL = all zero */, uint32_t* d_rv, uint32_t* d_wv,
                             uint32_t* d_final /* device, 2^mem_vars, or NULL */);

/* Memory checking in segments (tests/memcheck_segment_ref.py): the argument above with the image as a
 * COMMITTED column, so that a proof can start from the memory another proof ended in.  d_image is DEVICE memory, 2^mem_vars
 * words, never NULL; d_final (device, 2^mem_vars words, or NULL; it may be d_image itself, which is overwritten behind the
 * proof's last read of it) receives the final values fv - the next segment's image, without a host trip.  The proof commits eight columns, addr, rv, wv, iv, fv, rt, ft, m; its header differs from
 * lh_memcheck_prove's, so neither verifier takes the other's proof.  The verifier folds no image: 1 <= mem_vars < 31 and
 * the SRS are the limits; everything else is lh_memcheck_prove's.  A chain of segments is consistent when every segment
 * verifies and segment k + 1's image commitment (lh_memcheck_verify_segment) equals segment k's final commitment; a column's
 * commitment depends on nv = max(num_vars, mem_vars), so the segments of a chain share nv. */
lh_status lh_memcheck_prove_segment(lh_ctx*, const lh_srs*, const lh_memcheck_trace*, size_t num_vars, size_t mem_vars,
                                    const uint32_t* d_image, uint32_t* d_final, lh_transcript* t);

/* Spark (Lasso paper §4; the sparse commitment of Spartan): commit a sparse multilinear polynomial ONCE, prove its
 * evaluations at any number of points.  D in num_dims * dim_vars variables is given by 2^num_vars entries
 * (d_dims[0][k], .., d_dims[num_dims-1][k], d_val[k]): DEVICE columns uint32_t[2^num_vars] with values < 2^dim_vars and a
 * DEVICE column of 2^num_vars field elements (Montgomery form, as every device table here).
 *   D~(r_0, .., r_{num_dims-1}) = sum_k val[k] prod_j eq(r_j, dims[j][k]),   r_j = point[j dim_vars .. (j + 1) dim_vars)
 * Coordinate i of r_j belongs to bit i of dims[j]; the dense index is sum_j dims[j] << (j dim_vars); entries with the same
 * index add up; pad with val = 0 entries.  num_dims = 1 is a sparse vector, 2 a matrix.  Commit and open cost follows
 * 2^num_vars + 2^dim_vars, never 2^(num_dims dim_vars).  The protocol is specified in tests/spark_ref.py.
 *
 * lh_spark_commit copies the columns, counts the accesses (read_ts, final_cts) and commits the 1 + 3 num_dims polys
 * [val | dims | read_ts | final_cts], each zero-padded to nv = max(num_vars, dim_vars) variables.  The handle owns its
 * device memory (outside the proof arena) and the commitment; it is freed by lh_spark_free or with its ctx, and may be
 * opened any number of times: an opening runs no counter, no sort and no MSM over the committed columns.
 * lh_spark_commitment: the commitment bytes - the identity mask (one field element, big-endian as on a transcript), then the
 * non-identity points; out NULL: *len alone; else *len is the room in and the length out.
 * lh_spark_open appends the proof of D~(point) to t and returns the value in *out_value (point and value: HOST lh_fr).
 * Limits (LH_ERR_ARG with a message, checked on entry):
 *   1 <= num_dims <= LH_SPARK_MAX_DIMS       one sum-check term of num_dims + 1 <= LH_SC_MAX_FACTORS factors
 *   1 <= dim_vars <= LH_SPARK_MAX_DIM_VARS   an eq table per dimension: 2^dim_vars * 32 B
 *   1 <= num_vars < 31                       Lasso's bound: the access counters and their sort index entries by 32-bit words
 *   an index >= 2^dim_vars: "spark: index out of range" (the ctx stays usable)
 *   no NULL argument; not on a ctx inside a sharded prove, nor on one with a communicator of several ranks
 * LH_ERR_INVALID_PCS_PARAM when nv exceeds the SRS.  Multilinear KZG only. */
#define LH_SPARK_MAX_DIMS 3
#define LH_SPARK_MAX_DIM_VARS 24
typedef struct lh_spark_poly lh_spark_poly;
lh_status lh_spark_commit(lh_ctx*, const lh_srs*, size_t num_vars, size_t dim_vars, size_t num_dims,
                          const uint32_t* const* d_dims, const lh_fr* d_val, lh_spark_poly** out);
lh_status lh_spark_commitment(const lh_spark_poly*, uint8_t* out, size_t* len);
lh_status lh_spark_open(lh_ctx*, const lh_srs*, const lh_spark_poly*, const lh_fr* point /* num_dims * dim_vars */,
                        lh_fr* out_value, lh_transcript* t);
void lh_spark_free(lh_ctx*, lh_spark_poly*);
/* (lh_spark_verify: with the verifiers below; lh_debug_spark_e: with the debug entries) */

/* Spartan: prove that an R1CS instance is satisfied, over the Spark-committed matrices (tests/spartan_ref.py).
 * Instance: A, B, C of 2^dim_vars x 2^dim_vars, each 2^num_vars entries (d_row[k], d_col[k], d_val[k]) - DEVICE columns
 * uint32_t[2^num_vars] with values < 2^dim_vars and a DEVICE column of 2^num_vars field elements; the same num_vars for the
 * three; entries with the same position add up; pad with d_val = 0.  Assignment z of 2^dim_vars elements:
 * z[y] = w[y] for y < 2^(dim_vars-1) (the witness, DEVICE), z[2^(dim_vars-1) + i] = x[i] for i < num_public (HOST), 0 above;
 * the constant 1 is the caller's x[0].  Satisfied: (Az)[i] (Bz)[i] = (Cz)[i] for every row i.
 *
 * lh_r1cs_commit makes the key ONCE: the Spark commitments of A, B, C in the caller's entry order (dim 0 = row, dim 1 = col)
 * and, per matrix and direction, the entries sorted by row and by column (18 * 2^num_vars words of device memory outside
 * the proof arena).  The key owns its device memory; it is freed by lh_r1cs_free or with its ctx and proves any number of
 * assignments: a prove runs no sort.  lh_r1cs_commitment: the key bytes the verifier takes - the three lh_spark_commitment
 * blobs one after the other (A | B | C); out NULL: *len alone; else *len is the room in and the length out.
 * lh_spartan_prove appends the proof to t.  A witness that does not satisfy the instance is LH_ERR_ARG "spartan: the
 * witness does not satisfy K of the 2^l constraints": nothing is written to t and the ctx stays usable.
 * Limits (LH_ERR_ARG with a message, checked on entry):
 *   LH_SPARTAN_MIN_DIM_VARS <= dim_vars <= LH_SPARTAN_MAX_DIM_VARS   a witness half and a public half; Spark's bound
 *   1 <= num_vars < 31                                              Spark's
 *   1 <= num_public <= 2^(dim_vars - 1)
 *   an index >= 2^dim_vars: "spark: index out of range" (the ctx stays usable)
 *   no NULL argument; not on a ctx inside a sharded prove, nor on one with a communicator of several ranks
 * LH_ERR_INVALID_PCS_PARAM when max(num_vars, dim_vars) exceeds the SRS.  Multilinear KZG only. */
#define LH_SPARTAN_MIN_DIM_VARS 2
#define LH_SPARTAN_MAX_DIM_VARS 24
typedef struct lh_r1cs_matrix {
  const uint32_t* d_row;
  const uint32_t* d_col;
  const lh_fr* d_val;
} lh_r1cs_matrix;
typedef struct lh_r1cs_key lh_r1cs_key;
lh_status lh_r1cs_commit(lh_ctx*, const lh_srs*, size_t num_vars, size_t dim_vars, const lh_r1cs_matrix m[3], lh_r1cs_key** out);
lh_status lh_r1cs_commitment(const lh_r1cs_key*, uint8_t* out, size_t* len);
lh_status lh_spartan_prove(lh_ctx*, const lh_srs*, const lh_r1cs_key*, const lh_fr* d_w, const lh_fr* x /* host */,
                           size_t num_public, lh_transcript* t);
void lh_r1cs_free(lh_ctx*, lh_r1cs_key*);
/* (lh_spartan_verify: with the verifiers below; lh_debug_spartan_spmv: with the debug entries) */

/* Nova folding over an R1CS key, and the relaxed form of Spartan that closes a chain of folds (tests/nova_ref.py).
 * A relaxed instance is (C_W, C_E, x): C_W the commitment of w over dim_vars - 1 variables, C_E the one of the error vector E
 * over dim_vars variables, x the num_public public inputs with the relaxation scalar u = x[0]; its witness is (w, E) on the
 * DEVICE, its relation (Az)[i] (Bz)[i] = u (Cz)[i] + E[i] with z = (w, x, 0) as above.  It travels as ONE blob: the mask
 * element and the non-identity points of [C_W, C_E] as a commitment block writes them, then the elements of x - at most
 * LH_NOVA_INSTANCE_BYTES(num_public) bytes.  Every entry that makes an instance writes it to out_instance: *out_len is the room
 * in (at least LH_NOVA_INSTANCE_BYTES(num_public)) and the length out.
 *
 * lh_nova_instance: the fresh instance of an assignment that satisfies the key's instance as lh_spartan_prove takes it, with
 * x[0] = 1: E = 0, C_E the identity.  A witness that does not satisfy: LH_ERR_ARG "nova: the witness does not satisfy ...".
 * lh_nova_fold folds (instance1, d_w1, d_e1) and (instance2, d_w2, d_e2), either of them fresh or folded (d_e1 / d_e2 NULL:
 * zero), into d_w_out (2^(dim_vars-1) elements) and d_e_out (2^dim_vars) - which may be d_w1 and d_e1: a running accumulator
 * folds in place - and out_instance; the proof (the commitment block of the cross term: 96 bytes, 32 when it is zero) is
 * appended to t.  An input that fails its own relation is LH_ERR_ARG "nova: input K does not satisfy J of the 2^l
 * constraints": nothing is written to t and the ctx stays usable.  A fold runs no sort and no Spark kernel.  It does not check
 * that a blob's commitments open to the given vectors: the relaxed proof does.
 * lh_spartan_prove_relaxed proves a relaxed instance (d_e NULL: zero, for an instance whose C_E is the identity; a d_e given
 * beside such an instance has to be zero).  A witness that fails the relaxed relation, a NULL d_e beside a C_E that is a
 * point and a non-zero d_e beside the identity are LH_ERR_ARG before anything is written to t.
 * Limits and refusals are lh_spartan_prove's; also LH_ERR_ARG: a blob of the wrong length or with a mask out of range, two
 * instances with different numbers of public inputs.  Multilinear KZG only. */
#define LH_NOVA_INSTANCE_BYTES(num_public) (160 + 32 * (size_t)(num_public))
lh_status lh_nova_instance(lh_ctx*, const lh_srs*, const lh_r1cs_key*, const lh_fr* d_w, const lh_fr* x /* host */, size_t num_public,
                           uint8_t* out_instance, size_t* out_len);
lh_status lh_nova_fold(lh_ctx*, const lh_srs*, const lh_r1cs_key*, const uint8_t* instance1, size_t instance1_len,
                       const uint8_t* instance2, size_t instance2_len, const lh_fr* d_w1, const lh_fr* d_e1, const lh_fr* d_w2,
                       const lh_fr* d_e2, lh_fr* d_w_out, lh_fr* d_e_out, uint8_t* out_instance, size_t* out_len, lh_transcript* t);
lh_status lh_spartan_prove_relaxed(lh_ctx*, const lh_srs*, const lh_r1cs_key*, const uint8_t* instance, size_t instance_len,
                                   const lh_fr* d_w, const lh_fr* d_e, lh_transcript* t);
/* (lh_nova_fold_verify, lh_spartan_verify_relaxed: with the verifiers below; lh_debug_nova_*: with the debug entries) */

/* per-phase wall-clock of the last lh_lasso_prove on this ctx, milliseconds:
 * [witness, commit, surge, leaves+trees, gkr, evals, open_n, open_l, total] */
#define LH_LASSO_NUM_PHASES 9
lh_status lh_lasso_last_timing(lh_ctx*, double* out_ms);

/* ---------------------------------------------------------------- route options
 * The switches that decide WHICH code proves (never which bytes: every route yields the reference's transcript).  They
 * are per ctx; at lh_ctx_create each takes the value of the environment variable LH_<NAME IN UPPER CASE> when that is
 * set (LH_OPEN_SMALL_MIN_VARS=64 ...), else its default.  lh_ctx_set_option returns LH_ERR_ARG for an unknown name.
 *   open_small_min_vars  21   smallest batch opening (variables) whose largest quotient(s) are committed column by column
 *                             from 32-bit differences of the small-valued Lasso columns instead of from full-size
 *                             scalars (mkzg_open's column route; 64: never; below it an opening of at most four full
 *                             columns of >= 17 variables still takes it unless the option was set explicitly)
 *   open_small_depth     0    1 / 2: exactly that many column-wise quotient levels (0: chosen by cost)
 *   sc_eq_factoring      1    0: every sum-check round streams and binds its eq tables (the reference's shape) instead
 *                             of the factored form eq(y, x) = S_j eq(y_j, X) E_j[b]
 *   lasso_pack_ts        1    0: one MSM pass per read_ts column instead of packed pairs
 *   sc_tail              1    0: one kernel launch per sum-check round all the way down (no resident tail kernel)
 *   sc_tail_max_len      8192 longest table (entries) that enters the resident tail
 *   shard_exchange_log   19   sharded proofs: a sum-check goes on replicated once its residual tables hold <= 2^this
 *                             entries together (one all-gather), at the latest when the shard bits reach bit 0
 *   open_precommit       1    Lasso proofs of >= 2^this lookups (0: never, 1: always) run the column-wise quotient
 *                             commitments of their opening - MSMs over differences of witness columns, challenge-free - on
 *                             a helper ctx (own stream and host thread) beside the memory-checking sum-checks; the opening
 *                             then only combines their results
 *   open_precommit_stages 1   that precommit in two stages: the memory-bound half (column differences, digits, the sort of the
 *                             entries) starts as soon as the commit batch's bucket accumulation has left the chip and is
 *                             through before the product trees are built; the ALU-bound half (bucket accumulation, tails)
 *                             is released where the trees are built and runs beside the resident grand-product kernel.
 *                             0: all of it where the trees are built.  Sharded proofs and profiled proves always run one
 *                             stage (DESIGN.md sections 4 and 11)
 *   msm_window_tables    0   SRS levels of <= 2^this points get a window table on first use (2^(c w) multiples of every
 *                             base, W-fold the level's memory): the W windows of a full-width column then fill ONE
 *                             bucket set - one bucket reduction, no doublings.  Measured neutral at 2^24 lookups (shorter
 *                             reduction, longer bucket runs): off by default
 *   msm_half_batches     1    an MSM batch of >= 2^24 (point, window) entries runs as two halves: the latency-bound tails of
 *                             the first half (continuation levels, bucket reduction, window sums) run on a second stream of
 *                             the ctx beside the second half's bucket accumulation; the jobs with the most entries per
 *                             bucket go last (csrc/msm.hip msm_pick_split).  0: one batch on one stream
 *   gkr_resident         1    the layers near the roots of a grand-product argument (tables of <= 2^14 entries, <= 16 trees)
 *                             run in ONE resident launch - layer loop, eq tables, rounds and final evaluations inside the
 *                             kernel (kernels_gkr.hip); 0: one sum-check per layer (eq kernels, launched rounds, a resident
 *                             tail each).  Needs sc_tail and sc_eq_factoring
 *   sc_pp_fold           1    sum-checks of the shape eq * sum_m c_m l_m r_m (the generic layers of the grand products):
 *                             the streaming rounds share one Montgomery reduction among four products and the first
 *                             binding round folds c_m into l_m (sc_round_pp_kernel); the leaf layers of the lookup-sized
 *                             trees, sum_p cs_p (l_p + k_p)(r_p + k_p), store cs_p (l_p + k_p) and r_p + k_p at their first
 *                             bind and go on as such rounds; 0: sc_round_e2_kernel / sc_round_rw_kernel in every round
 *                             2: the product-pair kernel in every streaming round of the generic layers WITHOUT the fold
 *                             (the coefficients are applied to the lane's value, the tables stay as they are; a test shape)
 *   hyrax_rows           1    a Hyrax commit runs every row of every poly through the row kernels (csrc/kernels_hyrax.hip: the
 *                             terms of a row go into one bucket set over the generators' window table, nothing waits on
 *                             the host between rows); 0: one job of the batched MSM per row (48 jobs per planning pass)
 *   brakedown_batch_commit 1  lh_brakedown_batch_commit runs its polys as ONE batch (a poly dimension on the load, column-hash
 *                             and Merkle-level kernels, the encoder over all rows; one allocation, one copy of the roots);
 *                             0: one commit per poly
 *   brakedown_staged_open 0   lh_brakedown_batch_open stages the encoded matrix of a commitment on the host once (kernel
 *                             bd_stage_columns + one copy) and reads the opened columns there; 0: one device-to-host copy
 *                             per column.  (The HyperPlonk and Lasso provers over Brakedown always stage.)
 *   brakedown_u32_gather 1    a column commit (lh_brakedown_commit_columns, the Lasso prover over Brakedown) runs the first
 *                             encoder stage of its u32 columns from the 4-byte entries themselves (kernel bd_gather_u32: 256 x
 *                             32-bit products, a group's sum unreduced, one reduction per output); 0: the generic bd_gather
 *                             on the message as loaded in Montgomery form.  Rows, trees and roots are bit-identical.
 *   logup_fused_leaves   1    lh_logup_gkr_prove makes the leaves of a side's fractions and the level above them in ONE launch
 *                             (csrc/kernels_logup.hip logup_leaves_up: the input side never reads a table of ones); 0: the
 *                             leaves in one launch, then one frac_up launch per fraction.  lh_memcheck_prove's two leaf
 *                             kernels follow the same switch (the level above the trees' and the fractions' leaves)
 *                             and so does lh_spark_open's leaf kernel (0: the leaves only, and every write leaf stored)
 *   comm_round           0    how the partial sums of a sharded sum-check round are combined over the ranks:
 *                             0 = ncclAllGather of every rank's sums + a one-thread sum-and-publish kernel;
 *                             1 = ONE collective: the round kernel leaves its sums as u64 lanes (32-bit limb | tag << 40),
 *                                 ncclAllReduce(ncclSum, ncclUint64) adds them straight into the pinned memory the host
 *                                 polls (a lane whose upper bits read R * tag is finished), the host reduces mod r;
 *                             2 = the same all-reduce into device memory, then a copy to the host.
 *                             Same proof bytes; which is faster has never been measured on more than one GPU
 * Values outside an option's range are refused (LH_ERR_ARG).
 * lh_lasso_last_route reports which of these routes the last Lasso prove on the ctx actually took, so that a byte
 * mismatch in the field can be bisected from the outside. */
lh_status lh_ctx_set_option(lh_ctx*, const char* name, int64_t value);
lh_status lh_ctx_get_option(lh_ctx*, const char* name, int64_t* out);
#define LH_LASSO_ROUTE_WORDS 24
typedef struct lh_lasso_route {
  uint32_t open_small_depth;    /* column-wise quotient levels of the opening (0: plain route) */
  uint32_t open_small_passes;   /* column passes (MSM jobs) of those levels */
  uint32_t eq_factored_rounds;  /* launched sum-check rounds with factored eq tables */
  uint32_t standard_rounds;     /* launched rounds on the standard path (eq tables streamed and bound) */
  uint32_t rw_leaf_rounds;      /* of the factored rounds: the read/write leaf-layer kernel (sc_round_rw) */
  uint32_t resident_tails;      /* resident tail launches */
  uint32_t resident_rounds;     /* rounds that ran inside them */
  uint32_t packed_ts_pairs;     /* read_ts columns committed two to a pass */
  uint32_t derived_commitments; /* E columns committed from their dim column's buckets */
  uint32_t sorted_dim_reuse;    /* dim columns whose MSM entry stream came from the access counters' sort */
  uint32_t sharded_rounds;      /* rounds that carried a collective (sharded proofs) */
  uint32_t shard_exchanges;     /* residual-table / tree-level / remainder exchanges (sharded proofs) */
  uint32_t window_table_jobs;   /* MSM jobs that ran over a window table (msm_window_tables) */
  uint32_t open_precommit;      /* 1: the opening's column-wise commitments were taken from the helper ctx (open_precommit) */
  uint32_t resident_layers;     /* grand-product layers that ran inside the resident multi-layer kernel (gkr_resident) */
  uint32_t pp_folds;            /* sum-checks whose batching coefficients were folded into the left factors (sc_pp_fold) */
  uint32_t msm_half_batches;    /* MSM batches that ran as two pipelined halves (msm_half_batches; the slot was msm29_batches,
                                   always 0 since round 5) */
  uint32_t open_shared_sums;    /* (column, point) pairs whose quad sums the batch opening's column rounds took from the
                                   evaluation passes of the same proof instead of summing again (LH_OPEN_SHARE_SUMS) */
  uint32_t open_precommit_staged; /* 1: the prove ran that precommit in two stages (open_precommit_stages) */
  uint32_t reserved[5];
} lh_lasso_route;
lh_status lh_lasso_last_route(lh_ctx*, lh_lasso_route* out);

/* ---------------------------------------------------------------- e: one proof sharded over 2^rho GPUs
 * (the reference is single-process, there is nothing to cite.)  Every table of 2^m
 * entries is split on `rho` index bits [shard_bit, shard_bit + rho): the rank whose id equals those
 * bits holds the 2^(m-rho) entries (hi || lo).  Sum-check pairs (bit 0) and GKR / quotient halves (top
 * bit) stay local; per round each rank contributes D partial sums, per MSM one partial point, and when
 * the shard bits reach bit 0 the residual tables (2^(m-shard_bit) entries) are exchanged once.
 *
 * Transport.  On a multi-GPU node the communicator is RCCL over xGMI (lh_ctx_set_comm_rccl): one process per
 * GPU, one ncclComm per ctx, every device-side exchange is an ncclAllGather enqueued on the ctx's stream (a
 * sharded sum-check round is [round kernel -> all-gather of the D partial sums -> sum-and-publish kernel],
 * no host round trip in between).  The 128-byte unique id comes from lh_rccl_unique_id on one rank and reaches
 * the others over the caller's control plane.  lh_ctx_set_comm takes caller-supplied collectives instead
 * (tests: gloo through torch.distributed, several ranks on one GPU); device gathers are then staged through
 * the host unless all_gather_device is given. */
typedef struct lh_comm {
  int rank, size; /* size = 2^rho */
  void* user;
  /* host buffers: recv holds size * bytes_per_rank bytes, rank-major; returns 0 or a negative lh_status */
  int (*all_gather)(void* user, const void* send, void* recv, size_t bytes_per_rank);
  /* optional (may be NULL): the same over DEVICE buffers, enqueued on hip_stream (the ctx's stream) */
  int (*all_gather_device)(void* user, const void* d_send, void* d_recv, size_t bytes_per_rank, void* hip_stream);
} lh_comm;
/* comm == NULL detaches.  shard_bit + rho >= chunk_bits is required by lh_lasso_prove_sharded. */
lh_status lh_ctx_set_comm(lh_ctx*, const lh_comm* comm, size_t shard_bit);
#define LH_RCCL_UNIQUE_ID_BYTES 128
/* ncclGetUniqueId: call on ONE rank, distribute the bytes to every rank */
lh_status lh_rccl_unique_id(uint8_t out[LH_RCCL_UNIQUE_ID_BYTES]);
/* ncclCommInitRank on the ctx's device (collective: every rank of the job calls it with the same id) */
lh_status lh_ctx_set_comm_rccl(lh_ctx*, int rank, int size, const uint8_t unique_id[LH_RCCL_UNIQUE_ID_BYTES],
                               size_t shard_bit);
/* MEASUREMENT AID, not a transport: every peer is a copy of this rank (device gathers are device copies, nothing leaves
 * the GPU).  Rank `rank` of a `size`-rank sharded proof then runs alone with exactly the kernels, sizes and exchange
 * volumes it has in the real job - the compute half of a scaling curve on one GPU (tools/sharded_rank_profile.py).  The
 * transcript lh_lasso_prove_sharded produces over it is NOT a valid proof (the sums are R times this rank's share). */
lh_status lh_ctx_set_comm_loopback(lh_ctx*, int rank, int size, size_t shard_bit);
/* collectives issued on this ctx since the communicator was attached: out[0] device-side (RCCL or
 * all_gather_device), out[1] host callback.  A job on RCCL shows out[1] == 0. */
lh_status lh_ctx_comm_stats(lh_ctx*, uint64_t out[2]);
/* the same by phase of the Lasso prove in progress when the collective was issued: out[2 p] collectives, out[2 p + 1]
 * bytes this rank contributed, p = 0..6 for witness (the access counters' exchange), commit, surge, leaves, gkr, evals,
 * open; p = 7: outside a Lasso prove.  reset != 0 clears the counters after reading.  (bench.py prints them next to
 * the N > 1 line so that a measured scaling curve can be read against the per-rank compute profile.) */
lh_status lh_ctx_comm_phase_stats(lh_ctx*, uint64_t out[16], int reset);
/* device memory of a ctx (diagnostics; bench.py prints it per rank on the N > 1 line): out[0] = high-water mark of the
 * ctx's workspace arena in bytes (the prover's temporaries; its helper ctx's arena included), out[1] = bytes the arena
 * holds from the device now, out[2] / out[3] = free / total bytes of the device as the runtime reports them (all processes) */
lh_status lh_ctx_memory_stats(lh_ctx*, uint64_t out[4]);
/* the compute units of the ctx's device: what the kernels size their capped grids by (8 workgroups per unit for the round
 * kernels) - a test that wants a launch to stride asks here */
lh_status lh_ctx_compute_units(lh_ctx*, size_t* out);
/* the CPUs next to the ctx's device: its PCI address ("0000:72:00.0") into bus_id and the kernel's list of the CPUs on its
 * NUMA node ("0-63,128-191", sysfs local_cpulist) into cpulist - empty where the system does not say.  A deployment binds
 * the thread that proves to them (one process per GPU, bound to the GPU's node): the small proofs are a few hundred PCIe
 * round trips between that thread and the device, each one longer across the socket interconnect (tools/numa_ab.sh on a
 * quiet host: 2^20 lookups 8.09 against 8.26 ms).  The library never changes a caller's affinity itself. */
lh_status lh_ctx_host_cpus(lh_ctx*, char* bus_id, size_t bus_id_cap, char* cpulist, size_t cpulist_cap);
/* Same proof bytes as lh_lasso_prove on one GPU - it IS lh_lasso_prove with every table a shard: the same kernels (eq-
 * factored rounds, leaf-layer kernel, derived / packed commitments, column-wise top quotient) run on the shards, with a
 * collective where a round's partial sums or an MSM's partial commitments are added.  d_dims_local[j]: THIS RANK'S shard
 * of chunk column j, device u32[2^(num_vars - rho)] in the shard layout (local index hi || lo <-> lookup (hi, rank, lo)).
 * The access counters (a rank in the global lookup order per address) repartition the lookups by address owner with
 * one personalised exchange per column and direction; no rank ever holds a whole column.  Multilinear KZG only. */
lh_status lh_lasso_prove_sharded(lh_ctx*, const lh_srs*, const lh_lasso_table*, size_t num_vars,
                                 const uint32_t* const* d_dims_local, lh_transcript* t);

/* ---------------------------------------------------------------- f1: HyperPlonk with LogUp lookups
 * HyperPlonk::prove (backend/hyperplonk.rs:164-291), single-phase form (lh_hyperplonk_prove_phases below runs the
 * phase loop with a synthesize callback): instance hashing and
 * instance polys (hyperplonk.rs:170-177,365-369), witness commit, lookup_compressed_polys /
 * lookup_m_polys / lookup_h_polys / permutation_z_polys (backend/hyperplonk/prover.rs:50-313), the
 * zero-check sum-check over the composed expression (prover.rs:330-386, preprocessor.rs:25-60), the
 * evaluations in pcs_query order (verifier.rs:147-180) and MultilinearKzg::batch_open.
 * Poly numbering inside expressions is the reference's: instance | preprocess | witness |
 * permutation | lookup m | lookup h | permutation z.  Challenge numbering: circuit challenges, then
 * beta, gamma, alpha. */
typedef struct lh_hp_lookup {
  const lh_expr* inputs; /* [width] */
  const lh_expr* tables; /* [width] */
  size_t width;
} lh_hp_lookup;
/* A lookup proven by the Lasso argument INSIDE HyperPlonk::prove, in place of LogUp's m / h polys and constraint
 * (hyperplonk.rs:211-252, preprocessor.rs:79-109) - north_star's "hyperplonk::prover Lasso/Surge memory-check".  The
 * reference snapshot has no Lasso code; the schedule is specified in oracle/pyref/hyperplonk.py (LassoLookup).
 * On every row k the circuit poly `output_poly` holds a[k] = g(T_1[dim_1[k]], ..) and `chunk_polys[j]` the chunk
 * index dim_j[k] < 2^chunk_bits (ordinary circuit polys, normally witness columns tied to the circuit by its own gates;
 * not instance polys).  The argument adds committed polys read_ts_j | E_i | final_cts_j, numbered after the
 * permutation z polys; they are committed in round n after the LogUp m commitments (identity-mask framing), the
 * argument runs after the zero-check, and ONE batch_open serves the zero-check's queries and every Lasso claim.
 * Requires chunk_bits <= num_vars; output_poly and chunk_polys must be preprocess or witness polys (index >=
 * num_instance_polys and < num_instance_polys + num_preprocess_polys + witness polys - prover and verifier check the same
 * range); all Lasso commitments of one proof share one identity mask of 63 bits, so the lookups of a circuit may commit
 * to at most LH_HP_LASSO_MAX_COMMITMENTS polys together (sum over the lookups of 2 * num_chunks + num_memories). */
#define LH_HP_LASSO_MAX_COMMITMENTS 63
typedef struct lh_hp_lasso_lookup {
  lh_lasso_table table;
  size_t output_poly;
  size_t chunk_polys[LH_LASSO_MAX_CHUNKS];
} lh_hp_lasso_lookup;
typedef struct lh_hp_param { /* HyperPlonkProverParam (hyperplonk.rs:38-55), device-resident */
  size_t num_vars;
  size_t num_instance_polys;
  const size_t* num_instances;             /* [num_instance_polys] */
  size_t num_preprocess_polys;
  const void* const* d_preprocess_polys;   /* device lh_fr[2^num_vars] each */
  size_t num_witness_polys;                /* of the single phase */
  size_t num_challenges;                   /* squeezed after the witness commitments */
  size_t num_lookups;
  const lh_hp_lookup* lookups;
  size_t num_permutation_polys;
  const size_t* permutation_poly_index;    /* sorted poly indices under the permutation argument */
  const void* const* d_permutation_polys;  /* device lh_fr[2^num_vars] each (preprocessor.rs:172-203) */
  size_t num_permutation_z_polys;
  lh_expr expression;                      /* compose() output (preprocessor.rs:25-60) */
  size_t num_lasso_lookups;                /* lookups proven by Lasso instead of LogUp (0: none) */
  const lh_hp_lasso_lookup* lasso_lookups;
} lh_hp_param;
/* instances[i]: host, num_instances[i] elements.  d_witness_polys: device tables of the phase.
 * LH_ERR_INVALID_SNARK "Invalid lookup input" if an input row is not in its table (prover.rs:176), or if a Lasso
 * lookup's chunk column holds a value >= 2^chunk_bits or its output column is not the table's value. */
lh_status lh_hyperplonk_prove(lh_ctx*, const lh_srs*, const lh_hp_param*, const lh_fr* const* instances,
                              const lh_fr* const* d_witness_polys, lh_transcript* t);

/* ONE HyperPlonk proof over the 2^rho ranks of the ctx's communicator (SURVEY.md 8e / BASELINE.json configs[4]: the
 * Keccak-f circuit on 8 GPUs): HyperPlonk::prove (backend/hyperplonk.rs:164-291) with every table a shard.  Same proof
 * bytes on every rank as lh_hyperplonk_prove on one GPU.  `pp`: num_vars is the circuit's; d_preprocess_polys,
 * d_permutation_polys and d_witness_polys are THIS RANK'S shards - device lh_fr[2^(num_vars - rho)] in the shard layout
 * of lh_lasso_prove_sharded (local index hi || lo <-> row (hi, rank, lo)); instances are the full lists on every rank.
 * What crosses ranks: partial commitments (one exchange per commit round), the zero-check's partial sums per round and
 * its residual tables once (piop/sum_check/classic.rs:90-141 over shards), the rows of polys queried at a rotation
 * (gathered once in round 0, classic.rs:104-126), the per-row products of the permutation argument (gathered once; the
 * prefix product in hypercube order, backend/hyperplonk/prover.rs:308-323, runs on every rank), the Lasso lookups'
 * exchanges and the shared batch opening's as in lh_lasso_prove_sharded.  Circuits with LogUp lookups (a global
 * sort-merge join, prover.rs:139-200) are refused with LH_ERR_ARG: they run as replicas.  Needs shard_bit >= 1,
 * shard_bit + rho >= the Lasso lookups' chunk_bits and num_vars > shard_bit + rho; multilinear KZG. */
/* this rank's shard of a full device table: local[hi || lo] = global[(hi, rank, lo)], n_local = n / 2^rho entries of
 * elem_bytes (4, 32 or 64) each - how a caller that holds whole polys makes the inputs of the sharded proves */
lh_status lh_shard_extract(lh_ctx*, const void* d_global, size_t n_local, size_t shard_bit, size_t rho, size_t rank,
                           size_t elem_bytes, void* d_local);
lh_status lh_hyperplonk_prove_sharded(lh_ctx*, const lh_srs*, const lh_hp_param*, const lh_fr* const* instances,
                                      const lh_fr* const* d_witness_polys_local, lh_transcript* t);

/* Multi-phase circuits: the phase loop of HyperPlonk::prove (backend/hyperplonk.rs:185-205).  Phase r calls
 * PlonkishCircuit::synthesize(r, challenges so far) (backend.rs:139) for num_witness_polys[r] polys, commits them and
 * squeezes num_challenges[r] challenges; Challenge(i) in expressions indexes the concatenation, then beta, gamma, alpha.
 * The param's num_witness_polys / num_challenges hold the totals over the phases. */
typedef struct lh_hp_circuit { /* the witness half of `&impl PlonkishCircuit<F>` */
  void* user;
  /* fills d_out_polys[0 .. num_out) with DEVICE pointers to 2^num_vars lh_fr tables that stay valid until the prove
   * returns; `challenges` are those of the earlier phases; returns 0 or a negative lh_status */
  int (*synthesize)(void* user, size_t round, const lh_fr* challenges, size_t num_challenges,
                    const void** d_out_polys, size_t num_out);
} lh_hp_circuit;
lh_status lh_hyperplonk_prove_phases(lh_ctx*, const lh_srs*, const lh_hp_param*, size_t num_phases,
                                     const size_t* num_witness_polys, const size_t* num_challenges,
                                     const lh_fr* const* instances, const lh_hp_circuit* circuit, lh_transcript* t);

/* ---------------------------------------------------------------- f1: verifiers (host only, no GPU, no lh_ctx)
 * The verify half of the trait surface: PolynomialCommitmentScheme::{verify, batch_verify}
 * (pcs/multilinear/kzg.rs:330-375, pcs/multilinear.rs:237-276), SumCheck::verify (classic.rs:242-272),
 * PlonkishBackend::verify (backend/hyperplonk.rs:293-362, hyperplonk/verifier.rs:39-182), and the verifier
 * of the Lasso argument specified in oracle/pyref/lasso.py.  Pairings: BN254 optimal ate
 * (MultiMillerLoop::pairings_product_is_identity, util/arithmetic.rs:24-33). */
typedef struct lh_g2 { uint64_t x_c0[4], x_c1[4], y_c0[4], y_c1[4]; } lh_g2; /* bn256::G2Affine, Montgomery; identity = 0 */
typedef struct lh_mkzg_vp lh_mkzg_vp; /* MultilinearKzgVerifierParams (kzg.rs:79-101): g1, g2, ss[i] = s_i * g2 */
/* the verifier half of lh_mkzg_setup: same trapdoor, generators (1,2) and the bn256 G2 generator */
lh_status lh_mkzg_vp_setup(const lh_fr* ss, size_t num_vars, lh_mkzg_vp** out);
lh_status lh_mkzg_vp_new(const lh_g1* g1, const lh_g2* g2, const lh_g2* ss, size_t num_vars, lh_mkzg_vp** out);
lh_status lh_mkzg_vp_export(const lh_mkzg_vp*, lh_g1* g1, lh_g2* g2, lh_g2* ss);
size_t lh_mkzg_vp_num_vars(const lh_mkzg_vp*);
void lh_mkzg_vp_free(lh_mkzg_vp*);
/* e(p_i, q_i) product == 1 */
lh_status lh_pairing_check(const lh_g1* ps, const lh_g2* qs, size_t n, int* out_is_identity);
/* LH_ERR_INVALID_PCS_OPEN "Invalid multilinear KZG open" on a failed check */
lh_status lh_mkzg_verify(const lh_mkzg_vp*, const lh_g1* comm, const lh_fr* point, size_t num_vars,
                         const lh_fr* eval, lh_transcript* t);
lh_status lh_mkzg_batch_verify(const lh_mkzg_vp*, size_t num_vars, const lh_g1* comms, size_t num_comms,
                               const lh_fr* points, size_t num_points, const lh_evaluation* evals,
                               size_t num_evals, lh_transcript* t);
/* prover_kind selects the round-message type (Evaluations / Coefficients).  Outputs the final claim and
 * the challenges x[num_vars]; LH_ERR_INVALID_SUMCHECK on an inconsistent round. */
lh_status lh_sumcheck_verify(int prover_kind, size_t num_vars, size_t degree, const lh_fr* sum,
                             lh_transcript* t, lh_fr* out_eval, lh_fr* out_x);
lh_status lh_lasso_verify(const lh_mkzg_vp*, const lh_lasso_table*, size_t num_vars, lh_transcript* t);
/* the verifier of lh_lasso_prove_batch (tests/lasso_batch_ref.py verify): the same argument refusals as the prover's that
 * need no device, LH_ERR_INVALID_PCS_PARAM when max(num_vars, max chunk_bits) exceeds the param; a proof that does not
 * verify is LH_ERR_INVALID_SNARK whichever piece finds it out (a sum-check round, the opening, bytes that are no point or no
 * field element, a proof that ends early) - the message keeps that piece's words */
lh_status lh_lasso_verify_batch(const lh_mkzg_vp* vp, const lh_lasso_table* const* tables, size_t num_tables, size_t num_vars,
                                lh_transcript* t);
/* verify_fractional_sum_check (piop/gkr/fractional_sum_check.rs:193-270), the host verifier of lh_gkr_fractional_prove:
 * claimed_*[b] NULL (None => the root is read from the proof) or a claim (Some => only hashed).  Outputs, each optional:
 * the roots p_0s[B], q_0s[B] (read or given - a caller that argues with fractions checks a relation between them), the
 * final claims p_xs[B], q_xs[B] and the point x[num_vars].  LH_ERR_INVALID_SUMCHECK when a layer does not match;
 * LH_ERR_ARG for num_batching = 0, num_vars = 0 or more fractions than one layer sum-check takes. */
lh_status lh_gkr_fractional_verify(size_t num_batching, size_t num_vars, const lh_fr* const* claimed_p_0s,
                                   const lh_fr* const* claimed_q_0s, lh_transcript* t, lh_fr* out_p_0s, lh_fr* out_q_0s,
                                   lh_fr* out_p_xs, lh_fr* out_q_xs, lh_fr* out_x);
/* the verifier of lh_logup_gkr_prove (tests/logup_gkr_ref.py verify; host only): d_inputs of the lookups are ignored and may
 * be NULL.  The same argument refusals as the prover's that need no device; LH_ERR_INVALID_PCS_PARAM when
 * max(num_vars, table_vars) exceeds the param; a proof that does not verify is LH_ERR_INVALID_SNARK whichever piece finds
 * it out.  The tables' multilinear extensions are evaluated here, O(width 2^table_vars) field operations per lookup. */
lh_status lh_logup_gkr_verify(const lh_mkzg_vp* vp, const lh_logup_lookup* lookups, size_t num_lookups, size_t num_vars,
                              size_t table_vars, lh_transcript* t);
/* the verifier of lh_memcheck_prove (tests/memcheck_ref.py verify; host only).  The same limits as the prover's;
 * LH_ERR_INVALID_PCS_PARAM when max(num_vars, mem_vars) exceeds the param; a proof that does not verify is
 * LH_ERR_INVALID_SNARK whichever piece finds it out.  The image's multilinear extension is evaluated here, 2^mem_vars field
 * operations. */
lh_status lh_memcheck_verify(const lh_mkzg_vp* vp, size_t num_vars, size_t mem_vars, const uint32_t* init, lh_transcript* t);
/* the verifier of lh_memcheck_prove_segment (tests/memcheck_segment_ref.py verify; host only; no work of order 2^mem_vars).
 * On LH_OK *image_commitment and *final_commitment (either may be NULL) are the commitments of iv and fv as read from the
 * proof: lh_g1 as everywhere at this ABI, affine Montgomery coordinates, the identity - the commitment of an all-zero
 * column - as (0, 0).  They are written only when the proof verifies.  Limits and errors as lh_memcheck_verify's without an
 * image. */
lh_status lh_memcheck_verify_segment(const lh_mkzg_vp* vp, size_t num_vars, size_t mem_vars, lh_transcript* t,
                                     lh_g1* image_commitment, lh_g1* final_commitment);
/* the verifier of lh_spark_open (tests/spark_ref.py verify; host only): `commitment` are the bytes of lh_spark_commitment,
 * `point` the num_dims * dim_vars coordinates, `value` the claimed D~(point).  The same limits as the prover's;
 * LH_ERR_INVALID_PCS_PARAM when max(num_vars, dim_vars) exceeds the param; a proof that does not verify, a proof of another
 * value and a malformed commitment (mask out of range, wrong length, a point off the curve) are LH_ERR_INVALID_SNARK.  The eq
 * tables' extensions come in closed form: no work of order 2^dim_vars. */
lh_status lh_spark_verify(const lh_mkzg_vp* vp, size_t num_vars, size_t dim_vars, size_t num_dims, const uint8_t* commitment,
                          size_t commitment_len, const lh_fr* point, const lh_fr* value, lh_transcript* t);
/* the verifier of lh_spartan_prove (tests/spartan_ref.py verify; host only): `commitment` are the bytes of
 * lh_r1cs_commitment, `x` the num_public public inputs.  The same limits as the prover's; LH_ERR_INVALID_PCS_PARAM when
 * max(num_vars, dim_vars) exceeds the param; a proof that does not verify and a malformed key are LH_ERR_INVALID_SNARK
 * "spartan: ...".  The public half of z~ costs num_public field operations, the matrices none: Spark proves their values. */
lh_status lh_spartan_verify(const lh_mkzg_vp* vp, size_t num_vars, size_t dim_vars, const uint8_t* commitment, size_t commitment_len,
                            const lh_fr* x, size_t num_public, lh_transcript* t);
/* the verifier of lh_nova_fold (tests/nova_ref.py fold_verify; host only, no pairing and no param): absorbs the key and the two
 * instances, reads the cross term's commitment from t, and writes the folded instance - the prover's, byte for byte - to
 * out_instance (*out_len: room in, length out).  Blobs that cannot be read, of different numbers of public inputs, or a proof
 * that ends early are LH_ERR_INVALID_SNARK "nova: ...".  Nothing in a fold is checked: the relaxed proof of the result is. */
lh_status lh_nova_fold_verify(size_t num_vars, size_t dim_vars, const uint8_t* commitment, size_t commitment_len, const uint8_t* instance1,
                              size_t instance1_len, const uint8_t* instance2, size_t instance2_len, uint8_t* out_instance, size_t* out_len,
                              lh_transcript* t);
/* the verifier of lh_spartan_prove_relaxed (tests/nova_ref.py verify_relaxed; host only): as lh_spartan_verify, with the
 * instance blob in place of x.  An instance whose C_E is the identity carries no opening of E and must have vE = 0. */
lh_status lh_spartan_verify_relaxed(const lh_mkzg_vp* vp, size_t num_vars, size_t dim_vars, const uint8_t* commitment, size_t commitment_len,
                                    const uint8_t* instance, size_t instance_len, size_t num_public, lh_transcript* t);
/* Batched Spartan, the verifier (tests/spartan_batch_ref.py verify; host only): num_instances >= 2 assignments of
 * ONE R1CS key in one proof.  batch_vars = ceil(log2 num_instances), K = 2^batch_vars; the instances num_instances <= i < K
 * are zero (z = 0 satisfies every R1CS), so any count is allowed.  The assignments are stacked instance-minor, Z[i + K y], the
 * instance index in the LOW batch_vars coordinates; one outer sum-check over batch_vars + dim_vars variables brings every
 * instance to one r_x, one inner sum-check over the eq-weighted combination of the assignments, ONE opening of the stacked
 * witness (batch_vars + dim_vars - 1 variables) and ONE set of three Spark openings finish it.  `commitment` are the bytes of
 * lh_r1cs_commitment, `x` the num_instances * num_public public inputs instance by instance; the public half costs
 * num_instances * num_public products.  Limits (LH_ERR_ARG with a message): lh_spartan_verify's; num_instances >= 2;
 * dim_vars + batch_vars <= LH_SPARTAN_BATCH_MAX_VARS (the rows of the largest sum-check).  LH_ERR_INVALID_PCS_PARAM when
 * max(num_vars, batch_vars + dim_vars - 1) exceeds the param; a proof that does not verify and a malformed key are
 * LH_ERR_INVALID_SNARK "spartan: ...".  The proofs are the specification's: the library has no device prover for them yet. */
#define LH_SPARTAN_BATCH_MAX_VARS 26
lh_status lh_spartan_verify_batch(const lh_mkzg_vp* vp, size_t num_vars, size_t dim_vars, const uint8_t* commitment, size_t commitment_len,
                                  const lh_fr* x, size_t num_instances, size_t num_public, lh_transcript* t);
typedef struct lh_hp_vparam { /* HyperPlonkVerifierParam (hyperplonk.rs:57-74) */
  size_t num_vars;
  size_t num_instance_polys;
  const size_t* num_instances;
  size_t num_witness_polys;
  size_t num_challenges;
  size_t num_lookups;
  size_t num_permutation_z_polys;
  lh_expr expression;
  size_t num_preprocess_polys;
  const lh_g1* preprocess_comms;
  size_t num_permutation_polys;
  const lh_g1* permutation_comms;
  size_t num_lasso_lookups;
  const lh_hp_lasso_lookup* lasso_lookups;
} lh_hp_vparam;
lh_status lh_hyperplonk_verify(const lh_mkzg_vp*, const lh_hp_vparam*, const lh_fr* const* instances,
                               lh_transcript* t);
/* multi-phase (hyperplonk.rs:309-316): per phase num_witness_polys[r] commitments are read, num_challenges[r] squeezed */
lh_status lh_hyperplonk_verify_phases(const lh_mkzg_vp*, const lh_hp_vparam*, size_t num_phases,
                                      const size_t* num_witness_polys, const size_t* num_challenges,
                                      const lh_fr* const* instances, lh_transcript* t);

/* ---------------------------------------------------------------- f3: Zeromorph over univariate KZG
 * PolynomialCommitmentScheme for Zeromorph<UnivariateKzg<Bn256>> (pcs/multilinear/zeromorph.rs:67-256 on top of
 * pcs/univariate/kzg.rs:23-36,161-378): a multilinear table of 2^n evaluations is committed as the coefficient
 * vector of a univariate polynomial against powers_of_s_g1 (2^n points instead of multilinear KZG's 2^(n+1)-1).
 * `poly_size` is the trim size (zeromorph.rs:90-108): commitments use powers[..poly_size], the final quotient of
 * an opening powers[size - poly_size..]. */
typedef struct lh_usrs lh_usrs; /* UnivariateKzgParam: powers_of_s_g1 on the device */
lh_status lh_ukzg_setup(lh_ctx*, const lh_fr* s, size_t poly_size, lh_usrs** out); /* kzg.rs:175-218, trapdoor explicit */
lh_status lh_usrs_upload(lh_ctx*, const lh_g1* powers_of_s_g1, size_t poly_size, lh_usrs** out);
lh_status lh_usrs_download(lh_ctx*, const lh_usrs*, lh_g1* powers_of_s_g1);
size_t lh_usrs_size(const lh_usrs*);
void lh_usrs_free(lh_ctx*, lh_usrs*);
lh_status lh_zeromorph_batch_commit(lh_ctx*, const lh_usrs*, size_t poly_size, const lh_fr* const* d_polys,
                                    size_t num_polys, size_t num_vars, lh_g1* out_comms);
/* zeromorph.rs:134-199: writes n quotient commitments, q_hat's commitment and the KZG proof pi */
lh_status lh_zeromorph_open(lh_ctx*, const lh_usrs*, size_t poly_size, const lh_fr* d_poly, size_t num_vars,
                            const lh_fr* point, lh_transcript* t);
lh_status lh_zeromorph_batch_open(lh_ctx*, const lh_usrs*, size_t poly_size, size_t num_vars,
                                  const lh_fr* const* d_polys, size_t num_polys, const lh_fr* points,
                                  size_t num_points, const lh_evaluation* evals, size_t num_evals, lh_transcript* t);
/* verifier half (host only): ZeromorphKzgVerifierParam = (g1, g2, [s]_2, [s^offset]_2) */
typedef struct lh_zm_vp lh_zm_vp;
lh_status lh_zeromorph_vp_setup(const lh_fr* s, size_t param_size, size_t poly_size, lh_zm_vp** out);
lh_status lh_zeromorph_vp_new(const lh_g1* g1, const lh_g2* g2, const lh_g2* s_g2, const lh_g2* s_offset_g2,
                              lh_zm_vp** out);
lh_status lh_zeromorph_vp_export(const lh_zm_vp*, lh_g1* g1, lh_g2* g2, lh_g2* s_g2, lh_g2* s_offset_g2);
void lh_zeromorph_vp_free(lh_zm_vp*);
/* LH_ERR_INVALID_PCS_OPEN "Invalid Zeromorph KZG open" on a failed pairing check (zeromorph.rs:215-247) */
lh_status lh_zeromorph_verify(const lh_zm_vp*, const lh_g1* comm, const lh_fr* point, size_t num_vars,
                              const lh_fr* eval, lh_transcript* t);
lh_status lh_zeromorph_batch_verify(const lh_zm_vp*, size_t num_vars, const lh_g1* comms, size_t num_comms,
                                    const lh_fr* points, size_t num_points, const lh_evaluation* evals,
                                    size_t num_evals, lh_transcript* t);

/* HyperPlonk<Zeromorph<UnivariateKzg<Bn256>>> (the reference's second tested backend configuration,
 * backend/hyperplonk.rs:426): same schedule as lh_hyperplonk_prove / lh_hyperplonk_verify with the other PCS */
/* the Lasso argument over Zeromorph (same protocol, oracle/pyref/lasso.py with pcs = zeromorph) */
lh_status lh_lasso_prove_zeromorph(lh_ctx*, const lh_usrs*, size_t poly_size, const lh_lasso_table*, size_t num_vars,
                                   const uint32_t* const* d_dims, lh_transcript* t);
lh_status lh_lasso_verify_zeromorph(const lh_zm_vp*, const lh_lasso_table*, size_t num_vars, lh_transcript* t);
lh_status lh_hyperplonk_prove_zeromorph(lh_ctx*, const lh_usrs*, size_t poly_size, const lh_hp_param*,
                                        const lh_fr* const* instances, const lh_fr* const* d_witness_polys,
                                        lh_transcript* t);
lh_status lh_hyperplonk_verify_zeromorph(const lh_zm_vp*, const lh_hp_vparam*, const lh_fr* const* instances,
                                         lh_transcript* t);
/* multi-phase circuits over Zeromorph: the phase loop of backend/hyperplonk.rs:185-205 / 309-316 is generic over the PCS
 * (the reference instantiates HyperPlonk<Zeromorph<..>> at hyperplonk.rs:426); arguments as lh_hyperplonk_prove_phases /
 * lh_hyperplonk_verify_phases */
lh_status lh_hyperplonk_prove_phases_zeromorph(lh_ctx*, const lh_usrs*, size_t poly_size, const lh_hp_param*,
                                               size_t num_phases, const size_t* num_witness_polys,
                                               const size_t* num_challenges, const lh_fr* const* instances,
                                               const lh_hp_circuit* circuit, lh_transcript* t);
lh_status lh_hyperplonk_verify_phases_zeromorph(const lh_zm_vp*, const lh_hp_vparam*, size_t num_phases,
                                                const size_t* num_witness_polys, const size_t* num_challenges,
                                                const lh_fr* const* instances, lh_transcript* t);

/* ---------------------------------------------------------------- f3b: univariate KZG on its own, Gemini over it
 * PolynomialCommitmentScheme for UnivariateKzg<Bn256> (pcs/univariate/kzg.rs:161-555, with the SHPLONK-style batched
 * opening of several polys at several points) and for Gemini<UnivariateKzg<Bn256>> (pcs/multilinear/gemini.rs:29-211) over
 * the same lh_usrs.  `poly_size` is the trim size (kzg.rs:220-240): pp = powers[..poly_size].  A univariate poly is a
 * coefficient vector of `len` field elements on the device; the reference drops leading zero coefficients before it checks
 * a degree, here `len` itself must be <= poly_size (LH_ERR_INVALID_PCS_PARAM "Too large degree of poly to commit|open").
 * A commitment that is the identity cannot cross a transcript (util/transcript.rs:172-179): LH_ERR_TRANSCRIPT, as there. */
/* UnivariateKzg::batch_commit (kzg.rs:254-262) */
lh_status lh_ukzg_batch_commit(lh_ctx*, const lh_usrs*, size_t poly_size, const lh_fr* const* d_polys, const size_t* lens,
                               size_t num_polys, lh_g1* out_comms);
/* UnivariateKzg::open (kzg.rs:264-299): writes the commitment of poly div (X - point) */
lh_status lh_ukzg_open(lh_ctx*, const lh_usrs*, size_t poly_size, const lh_fr* d_poly, size_t len, const lh_fr* point,
                       lh_transcript* t);
/* UnivariateKzg::batch_open (kzg.rs:301-354): points are field elements, evals (poly, point, value) triples */
lh_status lh_ukzg_batch_open(lh_ctx*, const lh_usrs*, size_t poly_size, const lh_fr* const* d_polys, const size_t* lens,
                             size_t num_polys, const lh_fr* points, size_t num_points, const lh_evaluation* evals,
                             size_t num_evals, lh_transcript* t);
/* verifier half (host only): UnivariateKzgVerifierParam = (g1, g2, [s]_2) (kzg.rs:90-120) */
typedef struct lh_ukzg_vp lh_ukzg_vp;
lh_status lh_ukzg_vp_setup(const lh_fr* s, lh_ukzg_vp** out);
lh_status lh_ukzg_vp_new(const lh_g1* g1, const lh_g2* g2, const lh_g2* s_g2, lh_ukzg_vp** out);
lh_status lh_ukzg_vp_export(const lh_ukzg_vp*, lh_g1* g1, lh_g2* g2, lh_g2* s_g2);
void lh_ukzg_vp_free(lh_ukzg_vp*);
/* UnivariateKzg::verify (kzg.rs:366-378): LH_ERR_INVALID_PCS_OPEN "Invalid univariate KZG open" on a failed pairing check */
lh_status lh_ukzg_verify(const lh_ukzg_vp*, const lh_g1* comm, const lh_fr* point, const lh_fr* eval, lh_transcript* t);
/* UnivariateKzg::batch_verify (kzg.rs:380-419) */
lh_status lh_ukzg_batch_verify(const lh_ukzg_vp*, const lh_g1* comms, size_t num_comms, const lh_fr* points,
                               size_t num_points, const lh_evaluation* evals, size_t num_evals, lh_transcript* t);
/* Gemini::batch_commit (gemini.rs:56-76): the same bytes as lh_zeromorph_batch_commit */
lh_status lh_gemini_batch_commit(lh_ctx*, const lh_usrs*, size_t poly_size, const lh_fr* const* d_polys, size_t num_polys,
                                 size_t num_vars, lh_g1* out_comms);
/* Gemini::open (gemini.rs:78-138): writes n - 1 fold commitments, n evaluations, [q] and the KZG proof (96 n + 64 bytes) */
lh_status lh_gemini_open(lh_ctx*, const lh_usrs*, size_t poly_size, const lh_fr* d_poly, size_t num_vars,
                         const lh_fr* point, lh_transcript* t);
/* Gemini::batch_open (gemini.rs:140-155, additive::batch_open) */
lh_status lh_gemini_batch_open(lh_ctx*, const lh_usrs*, size_t poly_size, size_t num_vars, const lh_fr* const* d_polys,
                               size_t num_polys, const lh_fr* points, size_t num_points, const lh_evaluation* evals,
                               size_t num_evals, lh_transcript* t);
/* the folds fs[1..] of that opening (gemini.rs:100-108), flat: fs[i] (2^(n-i) coefficients) behind fs[i-1], 2^n - 2 in all */
lh_status lh_gemini_folds(lh_ctx*, const lh_fr* d_poly, size_t num_vars, const lh_fr* point, lh_fr* d_out);
/* Gemini::verify / batch_verify (gemini.rs:165-211) */
lh_status lh_gemini_verify(const lh_ukzg_vp*, const lh_g1* comm, const lh_fr* point, size_t num_vars, const lh_fr* eval,
                           lh_transcript* t);
lh_status lh_gemini_batch_verify(const lh_ukzg_vp*, size_t num_vars, const lh_g1* comms, size_t num_comms,
                                 const lh_fr* points, size_t num_points, const lh_evaluation* evals, size_t num_evals,
                                 lh_transcript* t);
/* Lasso and HyperPlonk<Gemini<UnivariateKzg<Bn256>>> (backend/hyperplonk.rs:425): arguments as the _zeromorph entries */
lh_status lh_lasso_prove_gemini(lh_ctx*, const lh_usrs*, size_t poly_size, const lh_lasso_table*, size_t num_vars,
                                const uint32_t* const* d_dims, lh_transcript* t);
lh_status lh_lasso_verify_gemini(const lh_ukzg_vp*, const lh_lasso_table*, size_t num_vars, lh_transcript* t);
lh_status lh_hyperplonk_prove_gemini(lh_ctx*, const lh_usrs*, size_t poly_size, const lh_hp_param*,
                                     const lh_fr* const* instances, const lh_fr* const* d_witness_polys, lh_transcript* t);
lh_status lh_hyperplonk_verify_gemini(const lh_ukzg_vp*, const lh_hp_vparam*, const lh_fr* const* instances,
                                      lh_transcript* t);
lh_status lh_hyperplonk_prove_phases_gemini(lh_ctx*, const lh_usrs*, size_t poly_size, const lh_hp_param*,
                                            size_t num_phases, const size_t* num_witness_polys,
                                            const size_t* num_challenges, const lh_fr* const* instances,
                                            const lh_hp_circuit* circuit, lh_transcript* t);
lh_status lh_hyperplonk_verify_phases_gemini(const lh_ukzg_vp*, const lh_hp_vparam*, size_t num_phases,
                                             const size_t* num_witness_polys, const size_t* num_challenges,
                                             const lh_fr* const* instances, lh_transcript* t);

/* ---------------------------------------------------------------- f4: Brakedown (transparent, no SRS)
 * PolynomialCommitmentScheme for MultilinearBrakedown<bn256::Fr, Keccak256, BrakedownSpec1..6>
 * (pcs/multilinear/brakedown.rs:89-417, util/code/brakedown.rs): 2^num_vars evaluations as num_rows rows of row_len,
 * each row encoded by the expander code to codeword_len entries, the columns hashed with Keccak-256 into a Merkle tree.
 * The sparse matrices are drawn from a 32-byte seed by this library's sampler instead of a caller's
 * RngCore.  Commitments are 32-byte roots; they and the Merkle paths cross the transcript through lh_hash_transcript. */
typedef struct lh_hash_transcript {
  void* user;
  int (*write_hash)(void* user, const uint8_t* hash32); /* TranscriptWrite<Output<Keccak256>, F>, transcript.rs:259-265 */
  int (*read_hash)(void* user, uint8_t* out32);          /* TranscriptRead<Output<Keccak256>, F>, transcript.rs:249-257 */
} lh_hash_transcript;
/* the hash half of the built-in Keccak256Transcript: 32 raw bytes in the stream, not absorbed (transcript.rs:240-265).
 * LH_ERR_ARG for a callback table that is not the built-in transcript. */
lh_status lh_keccak_transcript_hash_io(lh_transcript* t, lh_hash_transcript* out);
typedef struct lh_brakedown_param lh_brakedown_param; /* MultilinearBrakedownParams (brakedown.rs:35-41) */
typedef struct lh_brakedown_comm lh_brakedown_comm;   /* MultilinearBrakedownCommitment (brakedown.rs:55-60) */
/* setup (brakedown.rs:101-110) with poly_size = 2^num_vars, spec 1..6.  ctx NULL: host only (a verifier's param);
 * with a ctx the matrices are also uploaded, transposed, for the device encoder.  LH_ERR_ARG where the reference's
 * code dimensions do not exist (num_vars 1 with specs 1 and 2). */
lh_status lh_brakedown_setup(lh_ctx* ctx, size_t num_vars, int spec, const uint8_t* seed32, lh_brakedown_param** out);
/* the parameters alone, without matrices (no seed, nothing sampled): param_info and trim only */
lh_status lh_brakedown_derive(size_t num_vars, int spec, lh_brakedown_param** out);
/* row_len, num_rows, codeword_len (LinearCodes, code/mod.rs), num_column_opening, num_proximity_testing */
lh_status lh_brakedown_param_info(const lh_brakedown_param*, size_t* row_len, size_t* num_rows, size_t* codeword_len,
                                  size_t* num_column_opening, size_t* num_proximity_testing);
/* trim (brakedown.rs:112-126): the param is its own prover and verifier param; LH_ERR_INVALID_PCS_PARAM unless
 * poly_size == 2^num_vars */
lh_status lh_brakedown_trim(const lh_brakedown_param*, size_t poly_size);
void lh_brakedown_param_free(lh_brakedown_param*);
/* LinearCodes::encode (code/brakedown.rs:88-125) on the host: msg has row_len entries, out codeword_len */
lh_status lh_brakedown_encode(const lh_brakedown_param*, const lh_fr* msg, lh_fr* out);
/* commit / batch_commit (brakedown.rs:128-210): the rows and the tree stay on the ctx's device in the commitment.
 * batch_commit (option brakedown_batch_commit 1) runs the polys of the batch through the launches of one commit - rows, trees
 * and roots bit-identical to a commit per poly - into one device allocation that the last commitment of the batch frees. */
lh_status lh_brakedown_commit(lh_ctx*, const lh_brakedown_param*, const lh_fr* d_poly, size_t num_vars,
                              lh_brakedown_comm** out);
lh_status lh_brakedown_batch_commit(lh_ctx*, const lh_brakedown_param*, const lh_fr* const* d_polys, size_t num_polys,
                                    size_t num_vars, lh_brakedown_comm** out);
/* The commits of lh_brakedown_batch_commit of columns that are shorter than 2^num_vars or hold 32-bit integers, without a
 * field-element table per column: column i is lens[i] <= 2^num_vars entries on the device (d_cols[i] may be NULL when
 * lens[i] == 0), lh_fr in Montgomery form (LH_BD_COLUMN_FR) or uint32_t (LH_BD_COLUMN_U32), and is committed as the table
 * zero-padded to the param's num_vars.  Rows, trees and roots are bit-identical to lh_brakedown_batch_commit of those tables
 * (both values of option brakedown_u32_gather); one device allocation that the last commitment of the set frees. */
#define LH_BD_COLUMN_FR 0
#define LH_BD_COLUMN_U32 1
lh_status lh_brakedown_commit_columns(lh_ctx*, const lh_brakedown_param*, const void* const* d_cols, const int* kinds,
                                      const size_t* lens, size_t num_cols, lh_brakedown_comm** out);
lh_status lh_brakedown_comm_root(const lh_brakedown_comm*, uint8_t* out32); /* AsRef<[Output<H>]> (brakedown.rs:83-87) */
/* MultilinearBrakedownCommitment::rows (brakedown.rs:70-72): num_rows x codeword_len, row-major, a download */
lh_status lh_brakedown_comm_rows(lh_ctx*, const lh_brakedown_comm*, lh_fr* out);
/* the device address of the rows (tests: a change made after commit) */
lh_status lh_brakedown_comm_rows_device(const lh_brakedown_comm*, lh_fr** d_out);
/* the Merkle tree, a download: (2 << ceil(log2 codeword_len)) - 1 digests of 32 bytes, the leaves first, the root last */
lh_status lh_brakedown_comm_tree(lh_ctx*, const lh_brakedown_comm*, uint8_t* out);
/* the staged matrix of the open (kernel bd_stage_columns, then one copy): codeword_len x num_rows, column-major, i.e. the
 * transpose of lh_brakedown_comm_rows */
lh_status lh_brakedown_comm_stage(lh_ctx*, const lh_brakedown_param*, const lh_brakedown_comm*, lh_fr* out);
void lh_brakedown_comm_free(lh_brakedown_comm*);
/* open (brakedown.rs:212-276) */
lh_status lh_brakedown_open(lh_ctx*, const lh_brakedown_param*, const lh_fr* d_poly, size_t num_vars,
                            lh_brakedown_comm* comm, const lh_fr* point, lh_transcript* t, lh_hash_transcript* ht);
/* batch_open (brakedown.rs:278-300): one open per evaluation, in order.  Option brakedown_staged_open 1: the encoded
 * matrix of a commitment crosses to pinned host memory once and the columns of all its opens (consecutive evaluations of
 * one poly) are read there, instead of one device-to-host copy per column; the bytes written are the same. */
lh_status lh_brakedown_batch_open(lh_ctx*, const lh_brakedown_param*, size_t num_vars, const lh_fr* const* d_polys,
                                  lh_brakedown_comm* const* comms, size_t num_polys, const lh_fr* points,
                                  size_t num_points, const lh_evaluation* evals, size_t num_evals, lh_transcript* t,
                                  lh_hash_transcript* ht);
/* read_commitments (brakedown.rs:302-313): num roots of 32 bytes */
lh_status lh_brakedown_read_commitments(const lh_brakedown_param*, size_t num, lh_hash_transcript* ht, uint8_t* out);
/* verify (brakedown.rs:315-396), host only; LH_ERR_INVALID_PCS_OPEN with "Proximity failure",
 * "Invalid merkle tree opening" or "Consistency failure" */
lh_status lh_brakedown_verify(const lh_brakedown_param*, const uint8_t* root32, const lh_fr* point, size_t num_vars,
                              const lh_fr* eval, lh_transcript* t, lh_hash_transcript* ht);
/* batch_verify (brakedown.rs:398-417): one verify per evaluation; roots: num_comms x 32 bytes */
lh_status lh_brakedown_batch_verify(const lh_brakedown_param*, size_t num_vars, const uint8_t* roots, size_t num_comms,
                                    const lh_fr* points, size_t num_points, const lh_evaluation* evals,
                                    size_t num_evals, lh_transcript* t, lh_hash_transcript* ht);
/* HyperPlonk over Brakedown (backend/hyperplonk.rs:421-426 runs HyperPlonk over this scheme too).  The
 * arguments of the _zeromorph variants with the param in place of the SRS, the commitments of the preprocess and
 * permutation polys (made once with lh_brakedown_batch_commit; NULL only when there are none) in place of nothing - an
 * opening needs the commitment itself - and the hash transcript.  A commit round writes the raw roots through `ht` and
 * changes no Fiat-Shamir state; the batch opening is one open per evaluation in pcs_query order, over the staged matrix.
 * The witness, m, h and z commitments of the proof are batch commits into the ctx's arena, released when the prove
 * returns.  LH_ERR_ARG for a circuit with Lasso lookups (num_lasso_lookups != 0), for a ctx inside a sharded prove and for a
 * circuit whose num_vars is not the param's. */
lh_status lh_hyperplonk_prove_brakedown(lh_ctx*, const lh_brakedown_param*, const lh_hp_param* pp,
                                        lh_brakedown_comm* const* preprocess_comms,
                                        lh_brakedown_comm* const* permutation_comms, const lh_fr* const* instances,
                                        const lh_fr* const* d_witness_polys, lh_transcript* t, lh_hash_transcript* ht);
lh_status lh_hyperplonk_prove_phases_brakedown(lh_ctx*, const lh_brakedown_param*, const lh_hp_param* pp,
                                               lh_brakedown_comm* const* preprocess_comms,
                                               lh_brakedown_comm* const* permutation_comms, size_t num_phases,
                                               const size_t* num_witness_polys, const size_t* num_challenges,
                                               const lh_fr* const* instances, const lh_hp_circuit* circuit, lh_transcript* t,
                                               lh_hash_transcript* ht);
/* host only.  The roots of the preprocess and permutation polys come as arguments (32 bytes each; NULL only when there
 * are none): hvp's preprocess_comms / permutation_comms are ignored and may be NULL.  Ends in lh_brakedown_verify's check
 * once per evaluation: LH_ERR_INVALID_PCS_OPEN with its messages, LH_ERR_INVALID_SNARK from the zero-check. */
lh_status lh_hyperplonk_verify_brakedown(const lh_brakedown_param*, const lh_hp_vparam* hvp, const uint8_t* preprocess_roots,
                                         const uint8_t* permutation_roots, const lh_fr* const* instances, lh_transcript* t,
                                         lh_hash_transcript* ht);
lh_status lh_hyperplonk_verify_phases_brakedown(const lh_brakedown_param*, const lh_hp_vparam* hvp,
                                                const uint8_t* preprocess_roots, const uint8_t* permutation_roots,
                                                size_t num_phases, const size_t* num_witness_polys,
                                                const size_t* num_challenges, const lh_fr* const* instances, lh_transcript* t,
                                                lh_hash_transcript* ht);
/* Lasso over Brakedown: the arguments of lh_lasso_prove_zeromorph / lh_lasso_verify_zeromorph with the param in place of
 * the SRS, and the hash transcript.  The schedule is oracle/pyref/lasso.py's over this scheme: the mask element of the
 * commitment framing (always zero: the root of a zero column is a root like any other), then the 1 + 3 c + alpha roots
 * a | dim | read_ts | E | final_cts through `ht` (E_i of an identity subtable is dim_j: committed once, its root written
 * twice), the argument, and one open per evaluation (1 + 3 c + 2 alpha of them) over the staged matrix.  The columns are
 * committed as ONE batch from their 32-bit forms (lh_brakedown_commit_columns) into the ctx's arena, released when the prove
 * returns; the openings combine from the commitments' own rows.  The param must be set up for exactly max(num_vars,
 * chunk_bits) variables: LH_ERR_ARG otherwise, and for a ctx inside a sharded prove.  The verifier is host only: a mask
 * other than zero is LH_ERR_INVALID_SNARK ("lasso: commitment mask out of range"), a param of another size
 * LH_ERR_INVALID_PCS_PARAM, then lasso_verify's and lh_brakedown_verify's errors, and bytes left in a built-in
 * Keccak256 transcript LH_ERR_INVALID_SNARK ("trailing bytes in proof"). */
lh_status lh_lasso_prove_brakedown(lh_ctx*, const lh_brakedown_param*, const lh_lasso_table* table, size_t num_vars,
                                   const uint32_t* const* d_dims, lh_transcript* t, lh_hash_transcript* ht);
lh_status lh_lasso_verify_brakedown(const lh_brakedown_param*, const lh_lasso_table* table, size_t num_vars, lh_transcript* t,
                                    lh_hash_transcript* ht);

/* ---------------------------------------------------------------- f4b: Ligero (Brakedown's scheme over Reed-Solomon rows)
 * The scheme of f4 with the one other code a LinearCodes trait (util/code.rs) is expected to have: a systematic
 * Reed-Solomon code of rate 2^-log_inv_rate (1..3) over the roots of unity of bn256::Fr, encoded by a number-theoretic
 * transform (the specification is tests/ligero_ref.py).  row_len = 2^row_vars, codeword_len = row_len <<
 * log_inv_rate; position i * row_len + j of a codeword is f(w_N^i w_K^j) for the f that takes the message on the K-th
 * roots, so the first row_len entries are the message.  The code is MDS: 487 / 309 / 258 column openings at rate 1/2, 1/4,
 * 1/8 where Spec6 opens 3 755.  row_vars LH_LIGERO_ROW_VARS_AUTO: the row length of the smallest proof (the smallest on a
 * tie).  No seed: the param holds the table of roots, and with a ctx a copy of it on the device, freed with the param.
 * LH_ERR_ARG: log_inv_rate outside 1..3, num_vars outside 1..26, row_vars > num_vars (unless AUTO), row_vars + log_inv_rate
 * > 28, NULL out.  The param is an lh_brakedown_param: every lh_brakedown_*, lh_lasso_*_brakedown and
 * lh_hyperplonk_*_brakedown entry takes it unchanged (option brakedown_u32_gather has nothing to act on and is ignored);
 * lh_ligero_derive is parameters only (param_info and trim).  The device encoder takes rows up to 2^22. */
#define LH_LIGERO_ROW_VARS_AUTO ((size_t)-1)
lh_status lh_ligero_setup(lh_ctx* ctx /* NULL: host only */, size_t num_vars, int log_inv_rate, size_t row_vars,
                          lh_brakedown_param** out);
lh_status lh_ligero_derive(size_t num_vars, int log_inv_rate, size_t row_vars, lh_brakedown_param** out);

/* ---------------------------------------------------------------- f5: the multilinear IPA (transparent AND additive)
 * PolynomialCommitmentScheme for MultilinearIpa<bn256::G1Affine> (pcs/multilinear/ipa.rs:23-337): no trusted setup, no
 * pairing, commitments are G1 points - so additive::batch_open, Lasso and HyperPlonk apply to it as to the KZG family.
 * The generators are this library's own hash-to-point under the reference's domain and messages (the
 * reference's hash_to_curve belongs to a curve-library branch whose bytes cannot be pinned).  MultilinearIpaParams is
 * prover and verifier param at once; `poly_size` is the trim size (ipa.rs:129-145: a prefix of g), a power of two >= 2.
 * An opening is 128 num_vars + 32 bytes.  An L or R that is the identity (a table whose upper half is zero) cannot cross
 * a transcript (util/transcript.rs:172-179): LH_ERR_TRANSCRIPT after the bytes written by then, as there; a zero
 * challenge (the reference unwraps its inverse) is LH_ERR_ARG. */
typedef struct lh_ipa_param lh_ipa_param; /* MultilinearIpaParams (ipa.rs:25-44) */
/* setup (ipa.rs:98-127), poly_size a power of two in 2 .. 2^32 (num_vars 0 is LH_ERR_ARG: the reference's verifier
 * asserts on it).  With a ctx g is derived by a kernel and stays on the device (prover param); ctx NULL: on the host
 * (verifier param).  A param with device bases derives its host copy on first use by a verifier. */
lh_status lh_ipa_setup(lh_ctx* ctx, size_t poly_size, lh_ipa_param** out);
void lh_ipa_param_free(lh_ctx* ctx, lh_ipa_param*); /* ctx may be NULL for a host-only param */
size_t lh_ipa_param_size(const lh_ipa_param*);      /* 2^num_vars */
/* MultilinearIpaParams::g / ::h (ipa.rs:37-43): g (size points; a download when they are on the device - ctx needed then)
 * and h; either may be NULL */
lh_status lh_ipa_param_download(lh_ctx* ctx, const lh_ipa_param*, lh_g1* g, lh_g1* h);
/* commit / batch_commit (ipa.rs:147-168); tables of fewer variables than the param are committed against a prefix of g
 * (= their zero-padded table).  LH_ERR_INVALID_PCS_PARAM "Too many variates to trim" / "Too many variates of poly to .." */
lh_status lh_ipa_batch_commit(lh_ctx*, const lh_ipa_param*, size_t poly_size, const lh_fr* const* d_polys, size_t num_polys,
                              size_t num_vars, lh_g1* out_comms);
/* open (ipa.rs:170-241): num_vars rounds of (L, R), then the last coefficient; num_vars must equal log2(poly_size) */
lh_status lh_ipa_open(lh_ctx*, const lh_ipa_param*, size_t poly_size, const lh_fr* d_poly, size_t num_vars,
                      const lh_fr* point, lh_transcript* t);
/* batch_open (ipa.rs:243-254, additive::batch_open) */
lh_status lh_ipa_batch_open(lh_ctx*, const lh_ipa_param*, size_t poly_size, size_t num_vars, const lh_fr* const* d_polys,
                            size_t num_polys, const lh_fr* points, size_t num_points, const lh_evaluation* evals,
                            size_t num_evals, lh_transcript* t);
/* verify / batch_verify (ipa.rs:269-316), host only: one MSM of 2 num_vars + 2^num_vars + 1 terms;
 * LH_ERR_INVALID_PCS_OPEN "Invalid multilinear IPA open" */
lh_status lh_ipa_verify(const lh_ipa_param*, size_t poly_size, const lh_g1* comm, const lh_fr* point, size_t num_vars,
                        const lh_fr* eval, lh_transcript* t);
lh_status lh_ipa_batch_verify(const lh_ipa_param*, size_t poly_size, size_t num_vars, const lh_g1* comms, size_t num_comms,
                              const lh_fr* points, size_t num_points, const lh_evaluation* evals, size_t num_evals,
                              lh_transcript* t);
/* the base fold of an opening's round (ipa.rs:216-222) as a primitive: d_out[j] = d_a[j] + s d_b[j], j < n, affine
 * (identity = (0,0)); d_out may be d_a */
lh_status lh_g1_axpy(lh_ctx*, const lh_g1* d_a, const lh_g1* d_b, size_t n, const lh_fr* s, lh_g1* d_out);
/* the row commitments of a Hyrax commit (hyrax.rs:199-220) as a primitive: out_rows[r] = sum_{c < row_len}
 * s[r row_len + c] d_bases[c] for the ceil(n / row_len) rows of a flat DEVICE array of n scalars - lh_fr in Montgomery form, or
 * uint32_t with every value < 2^bits (scalars_u32 != 0, bits in 1..32; larger values lose their upper bits).  A partial last
 * row counts as padded with zeros.  d_bases: row_len device points; out_rows: HOST, affine, the identity as (0, 0).  One
 * launch set for all rows (csrc/kernels_hyrax.hip); the window table of the bases is built in workspace memory per call
 * (lh_hyrax_batch_commit keeps the generators' on the param).  LH_ERR_ARG for row_len 0 or bits outside 1..32 */
lh_status lh_g1_rows_msm(lh_ctx*, const void* d_scalars, int scalars_u32, uint32_t bits, size_t n, size_t row_len,
                         const lh_g1* d_bases, lh_g1* out_rows);
/* MultilinearHyrax<bn256::G1Affine> on top of it (pcs/multilinear/hyrax.rs:23-321): a table of 2^num_vars entries as
 * num_chunks = 2^(num_vars - row_num_vars) rows of 2^row_num_vars, one IPA commitment per row, with
 * batch_num_vars = log2(next_pow2(poly_size batch_size)) and row_num_vars = ceil(batch_num_vars / 2).  MultilinearHyraxParams
 * is those dimensions and an IPA param of 2^row_num_vars: an lh_ipa_param here, with (poly_size, batch_size) as the trim
 * arguments of every entry.  A commitment is num_chunks points, row 0 first; `comms` arrays are commitment-major.  Polys
 * must have exactly the (trimmed) param's num_vars.  Lasso and HyperPlonk prove over Hyrax through the _hyrax entries
 * below. */
/* setup (hyrax.rs:121-137): LH_ERR_ARG unless poly_size is a power of two and 0 < batch_size <= poly_size; ctx as lh_ipa_setup */
lh_status lh_hyrax_setup(lh_ctx* ctx, size_t poly_size, size_t batch_size, lh_ipa_param** out);
/* the dimensions setup and trim derive (hyrax.rs:125-127); outputs may be NULL */
lh_status lh_hyrax_dims(size_t poly_size, size_t batch_size, size_t* num_vars, size_t* batch_num_vars, size_t* row_num_vars);
/* trim (hyrax.rs:139-167): LH_ERR_INVALID_PCS_PARAM "Too many variates to trim" when the param's rows are too short */
lh_status lh_hyrax_trim(const lh_ipa_param*, size_t poly_size, size_t batch_size, size_t* row_num_vars, size_t* num_chunks);
/* commit / batch_commit (hyrax.rs:169-221): every row of every poly in one call of the row kernels (option hyrax_rows;
 * 0: every row a job of one batched MSM - the same points); out_comms: num_polys x num_chunks points */
lh_status lh_hyrax_batch_commit(lh_ctx*, const lh_ipa_param*, size_t poly_size, size_t batch_size, const lh_fr* const* d_polys,
                                size_t num_polys, size_t num_vars, lh_g1* out_comms);
/* open (hyrax.rs:224-258): the row combination sum_r eq(hi)[r] row_r in one pass, then the IPA opening of it at lo */
lh_status lh_hyrax_open(lh_ctx*, const lh_ipa_param*, size_t poly_size, size_t batch_size, const lh_fr* d_poly, size_t num_vars,
                        const lh_fr* point, lh_transcript* t);
/* batch_open (hyrax.rs:260-271, additive::batch_open) */
lh_status lh_hyrax_batch_open(lh_ctx*, const lh_ipa_param*, size_t poly_size, size_t batch_size, size_t num_vars,
                              const lh_fr* const* d_polys, size_t num_polys, const lh_fr* points, size_t num_points,
                              const lh_evaluation* evals, size_t num_evals, lh_transcript* t);
/* verify / batch_verify (hyrax.rs:288-320), host only: the MSM of the row commitments by eq(hi), then the IPA's verify;
 * batch_verify sums the vector commitments chunk by chunk (sum_with_scalar, hyrax.rs:80-107) */
lh_status lh_hyrax_verify(const lh_ipa_param*, size_t poly_size, size_t batch_size, const lh_g1* comm, const lh_fr* point,
                          size_t num_vars, const lh_fr* eval, lh_transcript* t);
lh_status lh_hyrax_batch_verify(const lh_ipa_param*, size_t poly_size, size_t batch_size, size_t num_vars, const lh_g1* comms,
                                size_t num_comms, const lh_fr* points, size_t num_points, const lh_evaluation* evals,
                                size_t num_evals, lh_transcript* t);
/* Lasso over MultilinearHyrax: arguments as the _ipa entries plus batch_size after poly_size.  max(num_vars, chunk_bits)
 * must equal log2(poly_size) (LH_ERR_ARG otherwise: Hyrax commits only tables of the param's size); a param whose rows are
 * too short is LH_ERR_INVALID_PCS_PARAM "Too many variates to trim".  The commitments are vectors of num_chunks points,
 * framed as count * num_chunks points commitment-major: ceil(total / 63) identity masks first (mask k covers the positions
 * 63 k .. 63 k + 62), then the non-identity points; a mask with a bit at or above its width is LH_ERR_INVALID_SNARK
 * "commitment mask out of range".  With num_chunks = 1 this is the framing of every other scheme, bit for bit. */
lh_status lh_lasso_prove_hyrax(lh_ctx*, const lh_ipa_param*, size_t poly_size, size_t batch_size, const lh_lasso_table*,
                               size_t num_vars, const uint32_t* const* d_dims, lh_transcript* t);
lh_status lh_lasso_verify_hyrax(const lh_ipa_param*, size_t poly_size, size_t batch_size, const lh_lasso_table*, size_t num_vars,
                                lh_transcript* t);
/* HyperPlonk<MultilinearHyrax<bn256::G1Affine>> (backend/hyperplonk.rs:421-426): arguments as the _ipa entries plus
 * batch_size after poly_size (what HyperPlonk::setup hands Pcs::setup: preprocessor.rs:13-23, Python hyperplonk.batch_size).
 * The circuit's num_vars must equal log2(poly_size) (LH_ERR_ARG).  Every commitment is num_chunks points: lh_hp_vparam's
 * preprocess_comms / permutation_comms hold num_chunks points per poly, poly-major; the witness, m, h and z commitments are
 * written plainly, as the reference writes them, so a ROW of such a poly that is identically zero (an identity row
 * commitment) ends the prove with LH_ERR_TRANSCRIPT after the bytes written by then - a property of the reference's
 * transcript; the Lasso lookups' commitments are framed as in lh_lasso_prove_hyrax. */
lh_status lh_hyperplonk_prove_hyrax(lh_ctx*, const lh_ipa_param*, size_t poly_size, size_t batch_size, const lh_hp_param*,
                                    const lh_fr* const* instances, const lh_fr* const* d_witness_polys, lh_transcript* t);
lh_status lh_hyperplonk_verify_hyrax(const lh_ipa_param*, size_t poly_size, size_t batch_size, const lh_hp_vparam*,
                                     const lh_fr* const* instances, lh_transcript* t);
lh_status lh_hyperplonk_prove_phases_hyrax(lh_ctx*, const lh_ipa_param*, size_t poly_size, size_t batch_size, const lh_hp_param*,
                                           size_t num_phases, const size_t* num_witness_polys, const size_t* num_challenges,
                                           const lh_fr* const* instances, const lh_hp_circuit* circuit, lh_transcript* t);
lh_status lh_hyperplonk_verify_phases_hyrax(const lh_ipa_param*, size_t poly_size, size_t batch_size, const lh_hp_vparam*,
                                            size_t num_phases, const size_t* num_witness_polys, const size_t* num_challenges,
                                            const lh_fr* const* instances, lh_transcript* t);
/* Lasso and HyperPlonk<MultilinearIpa<bn256::G1Affine>> (backend/hyperplonk.rs:76-95): arguments as the _gemini entries */
lh_status lh_lasso_prove_ipa(lh_ctx*, const lh_ipa_param*, size_t poly_size, const lh_lasso_table*, size_t num_vars,
                             const uint32_t* const* d_dims, lh_transcript* t);
lh_status lh_lasso_verify_ipa(const lh_ipa_param*, size_t poly_size, const lh_lasso_table*, size_t num_vars, lh_transcript* t);
lh_status lh_hyperplonk_prove_ipa(lh_ctx*, const lh_ipa_param*, size_t poly_size, const lh_hp_param*,
                                  const lh_fr* const* instances, const lh_fr* const* d_witness_polys, lh_transcript* t);
lh_status lh_hyperplonk_verify_ipa(const lh_ipa_param*, size_t poly_size, const lh_hp_vparam*, const lh_fr* const* instances,
                                   lh_transcript* t);
lh_status lh_hyperplonk_prove_phases_ipa(lh_ctx*, const lh_ipa_param*, size_t poly_size, const lh_hp_param*, size_t num_phases,
                                         const size_t* num_witness_polys, const size_t* num_challenges,
                                         const lh_fr* const* instances, const lh_hp_circuit* circuit, lh_transcript* t);
lh_status lh_hyperplonk_verify_phases_ipa(const lh_ipa_param*, size_t poly_size, const lh_hp_vparam*, size_t num_phases,
                                          const size_t* num_witness_polys, const size_t* num_challenges,
                                          const lh_fr* const* instances, lh_transcript* t);

/* development / tests: the HIP source the runtime compiler (csrc/jit.cpp) is given for a register program - words
 * {op | dst << 4 | a.kind << 8 | b.kind << 10, a.idx | b.idx << 16} with op ADD 0, SUB 1, MUL 2, NEG 3, MOV 4 and operand
 * kinds register 0, table 1, constant 2 (csrc/dev.hpp PROG_*).  Host code only (no GPU needed): tests/test_jit_source.py
 * evaluates the emitted statements against the program.  *len = length of the text; `out` may be null. */
lh_status lh_debug_jit_source(const uint32_t* code, size_t num_instrs, uint32_t num_regs, uint32_t result_reg, int degree,
                              char* out, size_t cap, size_t* len);

/* development / tests: the device radix sort (csrc/sort.hip) and the Lasso access counters on their own, for
 * tests/test_gpu_sort.py.  A slab is one stable sort of n (key, u32 value) pairs by the key bits [first_bit, first_bit +
 * bits): whole keys are carried along, inputs are preserved, d_vals_in == NULL means values = positions 0 .. n - 1.
 * key_bytes 4: `count` slabs as one batch (one launch set per radix pass).  key_bytes 8: count == 1 and first_bit == 0.
 * Refused with LH_ERR_ARG before anything is launched: another key_bytes, bits == 0, first_bit + bits > 8 key_bytes, a
 * null pointer with n > 0.  Temporary storage comes from the ctx's arena; the call returns after the sorts have finished. */
typedef struct lh_debug_sort_slab {
  const void* d_keys_in;
  void* d_keys_out;
  const uint32_t* d_vals_in;
  uint32_t* d_vals_out;
  size_t n;
  uint32_t bits, first_bit;
} lh_debug_sort_slab;
lh_status lh_debug_sort_pairs(lh_ctx*, int key_bytes, const lh_debug_sort_slab* slabs, size_t count);
/* num_cols columns of n addresses below m: d_read_ts[c][i] = earlier accesses of d_dims[c][i] in column c (n entries),
 * d_final_cts[c][a] = accesses of a (m entries); d_keep_sorted / d_keep_index (both or either may be NULL, else one pointer
 * per column): the column in ascending (stable) order and the positions it came from.  An address >= m: LH_ERR_ARG. */
lh_status lh_debug_lasso_counters(lh_ctx*, const uint32_t* const* d_dims, size_t num_cols, size_t n, size_t m,
                                  uint32_t* const* d_read_ts, uint32_t* const* d_final_cts, uint32_t* const* d_keep_sorted,
                                  uint32_t* const* d_keep_index);
/* the witness kernels of lh_memcheck_prove on their own (trace, sizes and init as there): d_rt[2^num_vars] the previous-write
 * times, d_fv / d_ft[2^mem_vars] the final values and times, d_m[2^num_vars] the multiplicities of i - rt[i] (all device).
 * *out_bad = 1 when the trace is invalid (an address >= 2^mem_vars, a read that does not return the last value written); the
 * columns are then unspecified.  The call itself still returns LH_OK. */
lh_status lh_debug_memcheck_witness(lh_ctx*, const lh_memcheck_trace*, size_t num_vars, size_t mem_vars, const uint32_t* init,
                                    uint32_t* d_rt, uint32_t* d_fv, uint32_t* d_ft, uint32_t* d_m, int* out_bad);
/* the memory kernel of lh_spark_open on its own (csrc/kernels_spark.hip spark_e): d_E[j][k] = eq(r_j, d_dims[j][k]) for the
 * num_dims dimensions (DEVICE, 2^num_vars field elements each), *out_value = sum_k d_val[k] prod_j d_E[j][k] (host).  Shapes
 * and limits as lh_spark_commit; an index >= 2^dim_vars is LH_ERR_ARG "spark: index out of range". */
lh_status lh_debug_spark_e(lh_ctx*, size_t num_vars, size_t dim_vars, size_t num_dims, const uint32_t* const* d_dims,
                           const lh_fr* d_val, const lh_fr* point, lh_fr* const* d_E, lh_fr* out_value);
/* the keyed field sum of lh_spartan_prove on its own (csrc/kernels_spartan.hip spartan_spmv), the three matrices of the key
 * in one launch set: direction 0, d_out[m] = M_m d_x (sums by row); direction 1, d_out[m] = M_m^T d_x (sums by column).
 * d_x and every d_out[m]: DEVICE, 2^dim_vars field elements; d_out is overwritten in full. */
lh_status lh_debug_spartan_spmv(lh_ctx*, const lh_r1cs_key*, int direction, const lh_fr* d_x, lh_fr* const d_out[3]);
/* the kernels of lh_nova_fold on their own (csrc/kernels_nova.hip).  nova_spmv2: lh_debug_spartan_spmv with two right-hand sides
 * in one pass, d_out1[m] = M_m d_x1 and d_out2[m] = M_m d_x2 (d_x1 and d_x2 may be one vector).  nova_cross_term over 2^dim_vars
 * rows: d_t = mz1[0] mz2[1] + mz2[0] mz1[1] - u1 mz2[2] - u2 mz1[2] and out_bad[k] = the rows at which input k fails
 * mz[0] mz[1] = u mz[2] + e (d_e1 / d_e2 NULL: zero; u1, u2: host).  nova_fold: d_w_out = d_w1 + r d_w2 over 2^(dim_vars-1)
 * and d_e_out = d_e1 + r d_t + r^2 d_e2 over 2^dim_vars in one launch (d_e1 / d_e2 NULL: zero); the outputs may be the inputs. */
lh_status lh_debug_nova_spmv2(lh_ctx*, const lh_r1cs_key*, int direction, const lh_fr* d_x1, const lh_fr* d_x2, lh_fr* const d_out1[3],
                              lh_fr* const d_out2[3]);
lh_status lh_debug_nova_cross_term(lh_ctx*, size_t dim_vars, const lh_fr* const d_mz1[3], const lh_fr* const d_mz2[3], const lh_fr* d_e1,
                                   const lh_fr* d_e2, const lh_fr* u1, const lh_fr* u2, lh_fr* d_t, size_t out_bad[2]);
lh_status lh_debug_nova_fold(lh_ctx*, size_t dim_vars, const lh_fr* d_w1, const lh_fr* d_w2, lh_fr* d_w_out, const lh_fr* d_e1,
                             const lh_fr* d_t, const lh_fr* d_e2, lh_fr* d_e_out, const lh_fr* r);
/* the pass plan of one slab (host only, no GPU needed): the number of radix passes, the digit width of each (rb[passes ..
 * 8) = 0; `bits` above the key width count as the key width) and the temporary device bytes the sort takes */
lh_status lh_debug_sort_plan(size_t n, unsigned bits, int key_bytes, unsigned* passes, unsigned rb[8], size_t* temp_bytes);
/* the planning half of a batched MSM (host only, no GPU needed) for jobs of n[j] points whose scalars have bits[j] significant
 * bits; kinds[j]: 0 = field elements, 1 = a 32-bit column, >= 4 = a packed pair of 32-bit columns with that pack shift.
 * helper != 0: planned as on a helper ctx (never two halves).  via_prepare: through the handle of the two-call form
 * (prepare, then run) instead of the one-call batch.  *num_subs = 1 or 2 sub-batches; out[12 s ..] of sub-batch s: jobs,
 * entries, small-job entries, buckets, segments, windows, groups, window-sum shares, entries per accumulate thread, chunks,
 * segment size, plain reduction (0 / 1).  out holds 24 words. */
lh_status lh_debug_msm_plan(size_t num_jobs, const size_t* n, const uint32_t* bits, const uint32_t* kinds, int helper, int via_prepare,
                            uint64_t* out, size_t* num_subs);
/* the library's owners of device resources (csrc/owned.hpp; host only).  live_resources: how many hold a resource in this
 * process right now - out[0] device blocks, [1] pinned host blocks, [2] events, [3] streams (memory of lh_alloc is the
 * caller's and is not counted).  fail_acquire_after: the (n + 1)-th acquisition of an owner from now on fails with
 * LH_ERR_DEVICE, once; n < 0 turns a pending failure off.  Process-wide, for tests of the failure paths of creation entries. */
lh_status lh_debug_live_resources(uint64_t out[4]);
lh_status lh_debug_fail_acquire_after(int64_t n);

/* development / tests: the kernels that work on 32-bit columns without their field-element views (csrc/kernels_poly.hip,
 * "small-valued columns"), one host function per operation, for tests/test_gpu_u32_columns.py.  Pointers named d_ are
 * device memory of lh_alloc; field elements are passed as everywhere in this header.  `n` is the operation's size:
 *   INNER_PRODUCTS_SMALL        out_host[k] = <d_cols[k], d_weights>, n entries each
 *   INNER_PRODUCTS_SMALL_HALF   out_host[k] = <d_cols[k], eq(y)> over 2 n entries; d_weights = eq(y[1..]) (n entries), r0 = y0
 *   INNER_PRODUCTS_SMALL_QUADS  one column of 4 n entries, d_weights = e0 (2 n entries); out_host[0..3] = sum_b e0[b] col[2b],
 *                               sum_b e0[b] col[2b+1], sum_q (e0[2q] + e0[2q+1]) col[4q+2], the same with col[4q+3]
 *   INNER_PRODUCTS_QUADS        d_out[4 k + t] = sum_{q < n} d_weights[q] d_cols[k][4 q + t]; entries from lens[k] on are zero
 *   QUAD_SUMS                   the same sums of all the columns in one launch from d_weights = e0 (2 n entries):
 *                               d_out[4 k + t] = sum_{q < n} (e0[2q] + e0[2q+1]) d_cols[k][4 q + t]; zero from lens[k] on
 *   LINCOMB_MIXED               d_out[i] = sum_k w_fr[k] d_fr[k][i] + sum_k w[k] d_cols[k][i], i < n (zero from lens[k] on)
 *   LINCOMB_FOLD_SMALL          d_out[i] = (1 - r0) g[i] + r0 g[i + n], g = sum_k w[k] d_cols[k] (zero from lens[k] on), i < n;
 *                               *taken = 0 and nothing written when count is 0 or above 24
 *   LINCOMB_BIND2               d_out[i] = sum_k w[k] (d_cols[k][4i .. 4i+3] bound with (r0, r1)), i < 2 n; out_host[e] =
 *                               sum_{b < n} d_weights[b] d_out[2b + e], e = 0, 1
 *   SC_ROUND_BIND2              the same of one column with weight one; out_host[0] = sum_{b < n} d_weights[b] d_out[2b + 1]
 * Refused with LH_ERR_ARG before anything is launched: a null pointer that the operation reads or writes, n == 0, more inputs
 * than a launch takes (LINCOMB_MIXED: 8 tables and 24 columns, LINCOMB_BIND2: 24 columns), and for the operations that read a
 * column 16 bytes at a time (the two QUADS, QUAD_SUMS and the two BIND2) a column that is not 16-byte aligned or a length that is no
 * multiple of 4.  The call returns after the stream has drained. */
enum {
  LH_U32_INNER_PRODUCTS_SMALL = 0,
  LH_U32_INNER_PRODUCTS_SMALL_HALF = 1,
  LH_U32_INNER_PRODUCTS_SMALL_QUADS = 2,
  LH_U32_INNER_PRODUCTS_QUADS = 3,
  LH_U32_LINCOMB_MIXED = 4,
  LH_U32_LINCOMB_FOLD_SMALL = 5,
  LH_U32_LINCOMB_BIND2 = 6,
  LH_U32_SC_ROUND_BIND2 = 7,
  LH_U32_QUAD_SUMS = 9 /* (8 is not an operation: LH_ERR_ARG, like every other value) */
};
typedef struct lh_debug_u32_args {
  const uint32_t* const* d_cols; /* `count` columns */
  const size_t* lens;            /* their lengths in entries (the operations that say "lens" above) */
  const lh_fr* w;                /* their weights, host (LINCOMB_*) */
  size_t count;
  const lh_fr* d_weights;        /* the weight / eq table */
  size_t n;
  const lh_fr* const* d_fr;      /* LINCOMB_MIXED: num_fr tables of n field elements and their weights (host) */
  const lh_fr* w_fr;
  size_t num_fr;
  lh_fr r0, r1;
  lh_fr* d_out;
  lh_fr* out_host;
  int* taken;                    /* LINCOMB_FOLD_SMALL */
} lh_debug_u32_args;
lh_status lh_debug_u32_columns(lh_ctx*, int op, const lh_debug_u32_args*);
/* (development) the subtable-read step of the Lasso witness alone: d_out[i] = T[d_dim[i]] for a memory of `kind` over
 * chunks of `chunk_bits` bits, by exactly what a prove runs for that memory - the computed entry of a built-in kind, the
 * masked gather from the registered entries otherwise (an index >= 2^chunk_bits reads T[index mod 2^chunk_bits]: a prove
 * refuses such a column by its access counters).  IDENTITY copies.  Returns after the stream has drained.
 * tests/test_gpu_lasso_custom.py. */
lh_status lh_debug_lasso_subtable_read(lh_ctx*, uint32_t kind, uint32_t chunk_bits, const uint32_t* d_dim, size_t n,
                                       uint32_t* d_out);

/* ---------------------------------------------------------------- measurement (bench.py)
 * Per-kernel HIP-event timing on the ctx stream.  While enabled every instrumented launch is
 * synchronised, so whole-prove wall time is NOT representative; use a separate pass. */
typedef struct lh_prof_rec {
  char name[40];
  double ms;    /* HIP-event duration of the launch */
  double bytes; /* algorithmic bytes of the launch */
  double muls;  /* field multiplications of the launch */
  double items; /* work items of the launch */
} lh_prof_rec;
/* on = 1: every instrumented launch bracketed by HIP events and SYNCHRONISED (exact per-kernel durations, a slower prove: not
 * for a timed region).  on = 2: LIVE records - an event pair around every bucket-accumulation launch (the dominant kernel), on
 * the stream it is launched on, nothing waited for: usable inside a timed region.  The two halves of a pipelined MSM batch
 * run at the same time, so a launch's `ms` is its span and a record named "msm_accumulate0/batch" carries the span of all
 * launches of one batch (first start to last end) with their bytes / muls / items added up.  Also clears the record list. */
lh_status lh_profile_enable(lh_ctx*, int on);
/* copies up to `cap` records, returns the total number recorded in *count */
lh_status lh_profile_read(lh_ctx*, lh_prof_rec* out, size_t cap, size_t* count);

#ifdef __cplusplus
}
#endif
#endif /* LASSO_HIP_H */
