//! `extern "C"` declarations of include/lasso_hip.h.  NEVER COMPILED - see README.md.
//! Field elements and points cross by pointer cast: lh_fr = bn256::Fr, lh_g1 = bn256::G1Affine, lh_g2 = bn256::G2Affine.
#![allow(non_camel_case_types, dead_code)]
use halo2_curves::bn256::{Fr, G1Affine, G2Affine};
use std::os::raw::{c_char, c_int, c_void};

pub type lh_status = c_int;
pub const LH_OK: lh_status = 0;
pub const LH_ERR_INVALID_SUMCHECK: lh_status = -1;
pub const LH_ERR_INVALID_PCS_PARAM: lh_status = -2;
pub const LH_ERR_INVALID_PCS_OPEN: lh_status = -3;
pub const LH_ERR_INVALID_SNARK: lh_status = -4;
pub const LH_ERR_SERIALIZATION: lh_status = -5;
pub const LH_ERR_TRANSCRIPT: lh_status = -6;
pub const LH_ERR_DEVICE: lh_status = -7;
pub const LH_ERR_ARG: lh_status = -8;

pub const LH_SC_MAX_TERMS: usize = 48;
pub const LH_SC_MAX_FACTORS: usize = 4;
pub const LH_SC_EVALUATIONS: c_int = 0;
pub const LH_SC_COEFFICIENTS: c_int = 1;
pub const LH_LASSO_MAX_CHUNKS: usize = 8;
pub const LH_LASSO_MAX_MEMORIES: usize = 16;
pub const LH_LASSO_MAX_TERMS: usize = 16;
pub const LH_RCCL_UNIQUE_ID_BYTES: usize = 128;

#[repr(C)] pub struct lh_ctx { _p: [u8; 0] }
#[repr(C)] pub struct lh_srs { _p: [u8; 0] }
#[repr(C)] pub struct lh_usrs { _p: [u8; 0] }
#[repr(C)] pub struct lh_mkzg_vp { _p: [u8; 0] }
#[repr(C)] pub struct lh_spark_poly { _p: [u8; 0] }  // a committed sparse polynomial (lh_spark_commit)
#[repr(C)] pub struct lh_r1cs_key { _p: [u8; 0] }  // the key of an R1CS instance (lh_r1cs_commit)
#[repr(C)] pub struct lh_zm_vp { _p: [u8; 0] }

pub type FeCb = unsafe extern "C" fn(*mut c_void, *const Fr) -> c_int;
pub type FeOutCb = unsafe extern "C" fn(*mut c_void, *mut Fr) -> c_int;
pub type G1Cb = unsafe extern "C" fn(*mut c_void, *const G1Affine) -> c_int;
pub type G1OutCb = unsafe extern "C" fn(*mut c_void, *mut G1Affine) -> c_int;

#[repr(C)]
pub struct lh_transcript {
    pub user: *mut c_void,
    pub write_field_element: Option<FeCb>,
    pub common_field_element: Option<FeCb>,
    pub squeeze_challenge: Option<FeOutCb>,
    pub write_commitment: Option<G1Cb>,
    pub common_commitment: Option<G1Cb>,
    pub read_field_element: Option<FeOutCb>,
    pub read_commitment: Option<G1OutCb>,
}

pub type HashCb = unsafe extern "C" fn(*mut c_void, *const u8) -> c_int;
pub type HashOutCb = unsafe extern "C" fn(*mut c_void, *mut u8) -> c_int;

// TranscriptWrite / TranscriptRead<Output<Keccak256>, Fr> (transcript.rs:240-265): 32 raw bytes, not absorbed
#[repr(C)]
pub struct lh_hash_transcript {
    pub user: *mut c_void,
    pub write_hash: Option<HashCb>,
    pub read_hash: Option<HashOutCb>,
}

#[repr(C)]
pub struct lh_sop {
    pub num_terms: u32,
    pub global_eq: i32,
    pub coeff: [Fr; LH_SC_MAX_TERMS],
    pub num_factors: [u8; LH_SC_MAX_TERMS],
    pub factor: [[u8; LH_SC_MAX_FACTORS]; LH_SC_MAX_TERMS],
}

pub const LH_LOGUP_MAX_LOOKUPS: usize = 8;
pub const LH_LOGUP_MAX_WIDTH: usize = 8;
pub const LH_LOGUP_MAX_TABLE_VARS: usize = 24;
// one lookup of lh_logup_gkr_prove: `width` device input columns of 2^num_vars Fr, `width` host table columns of 2^table_vars
#[repr(C)] #[derive(Clone, Copy)]
pub struct lh_logup_lookup { pub width: u32, pub d_inputs: *const *const Fr, pub table: *const *const Fr }
pub const LH_LOGUP_COL_FR: u8 = 0;   // lh_fr[2^num_vars], Montgomery
pub const LH_LOGUP_COL_U32: u8 = 1;  // uint32_t[2^num_vars], any 32-bit value
// one lookup of lh_logup_gkr_prove_columns: input column j has the type kinds[j] says (kinds null: every column LH_LOGUP_COL_FR)
#[repr(C)] #[derive(Clone, Copy)]
pub struct lh_logup_columns {
    pub width: u32, pub d_inputs: *const *const c_void, pub kinds: *const u8, pub table: *const *const Fr,
}
pub const LH_MEMCHECK_MAX_INIT_VARS: usize = 24;
pub const LH_SPARK_MAX_DIMS: usize = 3;
pub const LH_SPARK_MAX_DIM_VARS: usize = 24;
pub const LH_SPARTAN_MIN_DIM_VARS: usize = 2;
pub const LH_SPARTAN_MAX_DIM_VARS: usize = 24;
pub const LH_SPARTAN_BATCH_MAX_VARS: usize = 26;
// one matrix of lh_r1cs_commit: three device columns of 2^num_vars entries (row, col: uint32_t; val: field elements)
#[repr(C)] #[derive(Clone, Copy)]
pub struct lh_r1cs_matrix { pub d_row: *const u32, pub d_col: *const u32, pub d_val: *const Fr }
// the trace of lh_memcheck_prove: three device columns of 2^num_vars uint32_t (cell, value before, value after)
#[repr(C)] #[derive(Clone, Copy)]
pub struct lh_memcheck_trace { pub d_addr: *const u32, pub d_rv: *const u32, pub d_wv: *const u32 }
// the operations of lh_memcheck_replay: three device columns of 2^num_vars uint32_t (cell, store != 0, word to store)
#[repr(C)] #[derive(Clone, Copy)]
pub struct lh_memcheck_ops { pub d_addr: *const u32, pub d_store: *const u32, pub d_val: *const u32 }

pub const LH_EX_CONSTANT: u32 = 0;
pub const LH_EX_IDENTITY: u32 = 1;
pub const LH_EX_LAGRANGE: u32 = 2;
pub const LH_EX_EQ_XY: u32 = 3;
pub const LH_EX_POLYNOMIAL: u32 = 4;
pub const LH_EX_CHALLENGE: u32 = 5;
pub const LH_EX_NEGATED: u32 = 6;
pub const LH_EX_SUM: u32 = 7;
pub const LH_EX_PRODUCT: u32 = 8;
pub const LH_EX_SCALED: u32 = 9;
#[repr(C)] #[derive(Clone, Copy)]
pub struct lh_expr_node { pub op: u32, pub a: i32, pub b: i32, pub reserved: u32, pub scalar: Fr }
#[repr(C)] #[derive(Clone, Copy)]
pub struct lh_expr { pub nodes: *const lh_expr_node, pub num_nodes: usize }

// (development) one stable sort of lh_debug_sort_pairs: keys u32 or u64 by key_bytes, d_vals_in null = positions
#[repr(C)] #[derive(Clone, Copy)]
pub struct lh_debug_sort_slab {
    pub d_keys_in: *const c_void, pub d_keys_out: *mut c_void, pub d_vals_in: *const u32, pub d_vals_out: *mut u32,
    pub n: usize, pub bits: u32, pub first_bit: u32,
}

// (development) lh_debug_u32_columns: the 32-bit column kernels one operation at a time (op = LH_U32_*)
pub const LH_U32_INNER_PRODUCTS_SMALL: i32 = 0;
pub const LH_U32_INNER_PRODUCTS_SMALL_HALF: i32 = 1;
pub const LH_U32_INNER_PRODUCTS_SMALL_QUADS: i32 = 2;
pub const LH_U32_INNER_PRODUCTS_QUADS: i32 = 3;
pub const LH_U32_LINCOMB_MIXED: i32 = 4;
pub const LH_U32_LINCOMB_FOLD_SMALL: i32 = 5;
pub const LH_U32_LINCOMB_BIND2: i32 = 6;
pub const LH_U32_SC_ROUND_BIND2: i32 = 7;
pub const LH_U32_QUAD_SUMS: i32 = 9;
#[repr(C)] #[derive(Clone, Copy)]
pub struct lh_debug_u32_args {
    pub d_cols: *const *const u32, pub lens: *const usize, pub w: *const Fr, pub count: usize,
    pub d_weights: *const Fr, pub n: usize,
    pub d_fr: *const *const Fr, pub w_fr: *const Fr, pub num_fr: usize,
    pub r0: Fr, pub r1: Fr, pub d_out: *mut Fr, pub out_host: *mut Fr, pub taken: *mut i32,
}

#[repr(C)] #[derive(Clone, Copy)]
pub struct lh_evaluation { pub poly: u32, pub point: u32, pub value: Fr }

pub const LH_SUBTABLE_IDENTITY: u32 = 0;
pub const LH_SUBTABLE_AND: u32 = 1;
pub const LH_SUBTABLE_XOR: u32 = 2;
pub const LH_SUBTABLE_OR: u32 = 3;
pub const LH_SUBTABLE_EQ: u32 = 4;
pub const LH_SUBTABLE_LTU: u32 = 5;
// caller-registered subtables (lh_subtable_register): kinds from LH_SUBTABLE_CUSTOM_BASE up; 6 .. 0xFF stay LH_ERR_ARG
pub const LH_SUBTABLE_CUSTOM_BASE: u32 = 0x100;
pub const LH_SUBTABLE_CUSTOM_MAX: usize = 64;
pub const LH_SUBTABLE_CUSTOM_MAX_BITS: u32 = 20;
#[repr(C)] #[derive(Clone, Copy)]
pub struct lh_lasso_table {
    pub num_chunks: u32,
    pub chunk_bits: u32,
    pub num_memories: u32,
    pub memory_chunk: [u32; LH_LASSO_MAX_MEMORIES],
    pub memory_subtable: [u32; LH_LASSO_MAX_MEMORIES],
    pub num_terms: u32,
    pub g_coeff: [Fr; LH_LASSO_MAX_TERMS],
    pub g_num_factors: [u8; LH_LASSO_MAX_TERMS],
    pub g_factor: [[u8; LH_SC_MAX_FACTORS]; LH_LASSO_MAX_TERMS],
}

#[repr(C)]
pub struct lh_comm {
    pub rank: c_int,
    pub size: c_int,
    pub user: *mut c_void,
    pub all_gather: Option<unsafe extern "C" fn(*mut c_void, *const c_void, *mut c_void, usize) -> c_int>,
    pub all_gather_device: Option<unsafe extern "C" fn(*mut c_void, *const c_void, *mut c_void, usize, *mut c_void) -> c_int>,
}

#[repr(C)]
pub struct lh_hp_lookup { pub inputs: *const lh_expr, pub tables: *const lh_expr, pub width: usize }
#[repr(C)] #[derive(Clone, Copy)]
pub struct lh_hp_lasso_lookup {
    pub table: lh_lasso_table,
    pub output_poly: usize,
    pub chunk_polys: [usize; LH_LASSO_MAX_CHUNKS],
}
#[repr(C)]
pub struct lh_hp_param {
    pub num_vars: usize,
    pub num_instance_polys: usize,
    pub num_instances: *const usize,
    pub num_preprocess_polys: usize,
    pub d_preprocess_polys: *const *const c_void,
    pub num_witness_polys: usize,
    pub num_challenges: usize,
    pub num_lookups: usize,
    pub lookups: *const lh_hp_lookup,
    pub num_permutation_polys: usize,
    pub permutation_poly_index: *const usize,
    pub d_permutation_polys: *const *const c_void,
    pub num_permutation_z_polys: usize,
    pub expression: lh_expr,
    pub num_lasso_lookups: usize,
    pub lasso_lookups: *const lh_hp_lasso_lookup,
}
#[repr(C)]
pub struct lh_hp_vparam {
    pub num_vars: usize,
    pub num_instance_polys: usize,
    pub num_instances: *const usize,
    pub num_witness_polys: usize,
    pub num_challenges: usize,
    pub num_lookups: usize,
    pub num_permutation_z_polys: usize,
    pub expression: lh_expr,
    pub num_preprocess_polys: usize,
    pub preprocess_comms: *const G1Affine,
    pub num_permutation_polys: usize,
    pub permutation_comms: *const G1Affine,
    pub num_lasso_lookups: usize,
    pub lasso_lookups: *const lh_hp_lasso_lookup,
}
#[repr(C)]
pub struct lh_hp_circuit {
    pub user: *mut c_void,
    pub synthesize: Option<unsafe extern "C" fn(*mut c_void, usize, *const Fr, usize, *mut *const c_void, usize) -> c_int>,
}

/// lh_lasso_route (include/lasso_hip.h): which routes the last Lasso prove on a ctx took
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct lh_lasso_route {
    pub open_small_depth: u32,
    pub open_small_passes: u32,
    pub eq_factored_rounds: u32,
    pub standard_rounds: u32,
    pub rw_leaf_rounds: u32,
    pub resident_tails: u32,
    pub resident_rounds: u32,
    pub packed_ts_pairs: u32,
    pub derived_commitments: u32,
    pub sorted_dim_reuse: u32,
    pub sharded_rounds: u32,
    pub shard_exchanges: u32,
    pub window_table_jobs: u32,
    pub open_precommit: u32,
    pub resident_layers: u32,
    pub pp_folds: u32,
    pub msm_half_batches: u32,
    pub open_shared_sums: u32,
    pub open_precommit_staged: u32,
    pub reserved: [u32; 5],
}

extern "C" {
    pub fn lh_last_error() -> *const c_char;
    pub fn lh_version() -> *const c_char;
    // context & memory
    pub fn lh_ctx_create(device_id: c_int, out: *mut *mut lh_ctx) -> lh_status;
    pub fn lh_ctx_destroy(ctx: *mut lh_ctx);
    pub fn lh_ctx_sync(ctx: *mut lh_ctx) -> lh_status;
    pub fn lh_ctx_stream(ctx: *mut lh_ctx) -> *mut c_void;
    pub fn lh_alloc(ctx: *mut lh_ctx, bytes: usize, d_out: *mut *mut c_void) -> lh_status;
    pub fn lh_free(ctx: *mut lh_ctx, d_ptr: *mut c_void) -> lh_status;
    pub fn lh_upload(ctx: *mut lh_ctx, d_dst: *mut c_void, src: *const c_void, bytes: usize) -> lh_status;
    pub fn lh_download(ctx: *mut lh_ctx, dst: *mut c_void, d_src: *const c_void, bytes: usize) -> lh_status;
    // Fr vectors / MultilinearPolynomial
    pub fn lh_fr_from_u64(ctx: *mut lh_ctx, d_in: *const u64, n: usize, d_out: *mut Fr) -> lh_status;
    pub fn lh_fr_from_u32(ctx: *mut lh_ctx, d_in: *const u32, n: usize, d_out: *mut Fr) -> lh_status;
    pub fn lh_fr_batch_invert(ctx: *mut lh_ctx, d_in: *const Fr, n: usize, d_out: *mut Fr) -> lh_status;
    pub fn lh_fix_var(ctx: *mut lh_ctx, d_in: *const Fr, n_in: usize, x: *const Fr, d_out: *mut Fr) -> lh_status;
    pub fn lh_eq_xy(ctx: *mut lh_ctx, y: *const Fr, num_vars: usize, d_out: *mut Fr) -> lh_status;
    pub fn lh_evaluate(ctx: *mut lh_ctx, d_polys: *const *const Fr, num_polys: usize, num_vars: usize,
                       point: *const Fr, out_evals: *mut Fr) -> lh_status;
    pub fn lh_lincomb(ctx: *mut lh_ctx, d_polys: *const *const Fr, w: *const Fr, num_polys: usize, n: usize,
                      d_out: *mut Fr) -> lh_status;
    // piop::sum_check, piop::gkr
    pub fn lh_sumcheck_prove(ctx: *mut lh_ctx, prover_kind: c_int, num_vars: usize, expr: *const lh_sop,
                             d_polys: *const *const Fr, num_polys: usize, ys: *const Fr, num_ys: usize,
                             sum: *const Fr, t: *mut lh_transcript, out_challenges: *mut Fr, out_evals: *mut Fr) -> lh_status;
    pub fn lh_sumcheck_prove_expr(ctx: *mut lh_ctx, num_vars: usize, expr: *const lh_expr, d_polys: *const *const Fr,
                                  num_polys: usize, challenges: *const Fr, num_challenges: usize, ys: *const Fr,
                                  num_ys: usize, sum: *const Fr, t: *mut lh_transcript, out_challenges: *mut Fr,
                                  out_evals: *mut Fr) -> lh_status;
    pub fn lh_sumcheck_verify(prover_kind: c_int, num_vars: usize, degree: usize, sum: *const Fr,
                              t: *mut lh_transcript, out_eval: *mut Fr, out_x: *mut Fr) -> lh_status;
    pub fn lh_gkr_fractional_prove(ctx: *mut lh_ctx, num_batching: usize, num_vars: usize,
                                   claimed_p_0s: *const *const Fr, claimed_q_0s: *const *const Fr,
                                   d_ps: *const *const Fr, d_qs: *const *const Fr, t: *mut lh_transcript,
                                   out_p_xs: *mut Fr, out_q_xs: *mut Fr, out_x: *mut Fr) -> lh_status;
    // util::arithmetic::msm
    pub fn lh_msm(ctx: *mut lh_ctx, d_scalars: *const Fr, d_bases: *const G1Affine, n: usize, out: *mut G1Affine) -> lh_status;
    pub fn lh_msm_u32(ctx: *mut lh_ctx, d_scalars: *const u32, d_bases: *const G1Affine, n: usize, out: *mut G1Affine) -> lh_status;
    // pcs::multilinear::kzg
    pub fn lh_srs_upload(ctx: *mut lh_ctx, eqs_flat: *const G1Affine, num_vars: usize, out: *mut *mut lh_srs) -> lh_status;
    pub fn lh_srs_num_vars(srs: *const lh_srs) -> usize;
    pub fn lh_srs_free(ctx: *mut lh_ctx, srs: *mut lh_srs);
    pub fn lh_mkzg_batch_commit(ctx: *mut lh_ctx, srs: *const lh_srs, d_polys: *const *const Fr, num_polys: usize,
                                num_vars: usize, out_comms: *mut G1Affine) -> lh_status;
    pub fn lh_mkzg_open(ctx: *mut lh_ctx, srs: *const lh_srs, d_poly: *const Fr, num_vars: usize, point: *const Fr,
                        t: *mut lh_transcript, out_eval: *mut Fr) -> lh_status;
    pub fn lh_mkzg_batch_open(ctx: *mut lh_ctx, srs: *const lh_srs, num_vars: usize, d_polys: *const *const Fr,
                              num_polys: usize, points: *const Fr, num_points: usize, evals: *const lh_evaluation,
                              num_evals: usize, t: *mut lh_transcript) -> lh_status;
    pub fn lh_mkzg_vp_new(g1: *const G1Affine, g2: *const G2Affine, ss: *const G2Affine, num_vars: usize,
                          out: *mut *mut lh_mkzg_vp) -> lh_status;
    pub fn lh_mkzg_vp_free(vp: *mut lh_mkzg_vp);
    pub fn lh_mkzg_verify(vp: *const lh_mkzg_vp, comm: *const G1Affine, point: *const Fr, num_vars: usize,
                          eval: *const Fr, t: *mut lh_transcript) -> lh_status;
    pub fn lh_mkzg_batch_verify(vp: *const lh_mkzg_vp, num_vars: usize, comms: *const G1Affine, num_comms: usize,
                                points: *const Fr, num_points: usize, evals: *const lh_evaluation, num_evals: usize,
                                t: *mut lh_transcript) -> lh_status;
    // Lasso
    pub fn lh_lasso_prove(ctx: *mut lh_ctx, srs: *const lh_srs, table: *const lh_lasso_table, num_vars: usize,
                          d_dims: *const *const u32, t: *mut lh_transcript) -> lh_status;
    pub fn lh_lasso_verify(vp: *const lh_mkzg_vp, table: *const lh_lasso_table, num_vars: usize,
                           t: *mut lh_transcript) -> lh_status;
    // lookups into several tables in one proof (at most LH_LASSO_BATCH_MAX_TABLES = 8): d_dims[t][j] is chunk column j of table t
    pub fn lh_lasso_prove_batch(ctx: *mut lh_ctx, srs: *const lh_srs, tables: *const *const lh_lasso_table, num_tables: usize,
                                num_vars: usize, d_dims: *const *const *const u32, t: *mut lh_transcript) -> lh_status;
    pub fn lh_lasso_verify_batch(vp: *const lh_mkzg_vp, tables: *const *const lh_lasso_table, num_tables: usize,
                                 num_vars: usize, t: *mut lh_transcript) -> lh_status;
    // LogUp-GKR: lookups by value into unstructured tables (tests/logup_gkr_ref.py); the verifier ignores d_inputs
    pub fn lh_logup_gkr_prove(ctx: *mut lh_ctx, srs: *const lh_srs, lookups: *const lh_logup_lookup, num_lookups: usize,
                              num_vars: usize, table_vars: usize, t: *mut lh_transcript) -> lh_status;
    // the same proof (same bytes, same verifier) from input columns of which some are uint32_t
    pub fn lh_logup_gkr_prove_columns(ctx: *mut lh_ctx, srs: *const lh_srs, lookups: *const lh_logup_columns,
                                      num_lookups: usize, num_vars: usize, table_vars: usize, t: *mut lh_transcript) -> lh_status;
    pub fn lh_logup_gkr_verify(vp: *const lh_mkzg_vp, lookups: *const lh_logup_lookup, num_lookups: usize, num_vars: usize,
                               table_vars: usize, t: *mut lh_transcript) -> lh_status;
    // read-write memory checking of a RAM trace (tests/memcheck_ref.py); init: host, 2^mem_vars words, or null (all zero)
    pub fn lh_memcheck_prove(ctx: *mut lh_ctx, srs: *const lh_srs, trace: *const lh_memcheck_trace, num_vars: usize,
                             mem_vars: usize, init: *const u32, t: *mut lh_transcript) -> lh_status;
    pub fn lh_memcheck_verify(vp: *const lh_mkzg_vp, num_vars: usize, mem_vars: usize, init: *const u32,
                              t: *mut lh_transcript) -> lh_status;
    // (development) its witness kernels on their own; *out_bad = 1: an invalid trace
    pub fn lh_debug_memcheck_witness(ctx: *mut lh_ctx, trace: *const lh_memcheck_trace, num_vars: usize, mem_vars: usize,
                                     init: *const u32, d_rt: *mut u32, d_fv: *mut u32, d_ft: *mut u32, d_m: *mut u32,
                                     out_bad: *mut i32) -> lh_status;
    // the trace from the operations, on the device: rv, wv and the final cells (d_image, d_final: device, or null)
    pub fn lh_memcheck_replay(ctx: *mut lh_ctx, ops: *const lh_memcheck_ops, num_vars: usize, mem_vars: usize,
                              d_image: *const u32, d_rv: *mut u32, d_wv: *mut u32, d_final: *mut u32) -> lh_status;
    // memory checking in segments (tests/memcheck_segment_ref.py): the image a committed device column; the verifier returns
    // the commitments of the image and of the final values (identity = (0, 0)), each may be null
    pub fn lh_memcheck_prove_segment(ctx: *mut lh_ctx, srs: *const lh_srs, trace: *const lh_memcheck_trace, num_vars: usize,
                                     mem_vars: usize, d_image: *const u32, d_final: *mut u32, t: *mut lh_transcript) -> lh_status;
    pub fn lh_memcheck_verify_segment(vp: *const lh_mkzg_vp, num_vars: usize, mem_vars: usize, t: *mut lh_transcript,
                                      image_commitment: *mut G1Affine, final_commitment: *mut G1Affine) -> lh_status;
    // Spark (tests/spark_ref.py): commit a sparse polynomial once - 2^num_vars entries (d_dims[j][k] < 2^dim_vars, d_val[k]),
    // device columns - and prove its evaluations at any number of points; the handle owns its device memory
    pub fn lh_spark_commit(ctx: *mut lh_ctx, srs: *const lh_srs, num_vars: usize, dim_vars: usize, num_dims: usize,
                           d_dims: *const *const u32, d_val: *const Fr, out: *mut *mut lh_spark_poly) -> lh_status;
    // out null: the length alone; else *len is the room in and the length out
    pub fn lh_spark_commitment(poly: *const lh_spark_poly, out: *mut u8, len: *mut usize) -> lh_status;
    // point: num_dims * dim_vars host coordinates; the proof is appended to t
    pub fn lh_spark_open(ctx: *mut lh_ctx, srs: *const lh_srs, poly: *const lh_spark_poly, point: *const Fr, out_value: *mut Fr,
                         t: *mut lh_transcript) -> lh_status;
    pub fn lh_spark_free(ctx: *mut lh_ctx, poly: *mut lh_spark_poly);
    pub fn lh_spark_verify(vp: *const lh_mkzg_vp, num_vars: usize, dim_vars: usize, num_dims: usize, commitment: *const u8,
                           commitment_len: usize, point: *const Fr, value: *const Fr, t: *mut lh_transcript) -> lh_status;
    // (development) the memory kernel of an opening on its own: d_E[j][k] = eq(r_j, d_dims[j][k]) and the value
    pub fn lh_debug_spark_e(ctx: *mut lh_ctx, num_vars: usize, dim_vars: usize, num_dims: usize, d_dims: *const *const u32,
                            d_val: *const Fr, point: *const Fr, d_E: *const *mut Fr, out_value: *mut Fr) -> lh_status;
    // Spartan (tests/spartan_ref.py): the key of an R1CS instance once - m: three matrices A, B, C -, then any number of proofs
    // of assignments z = (d_w, x, 0); the key owns its device memory
    pub fn lh_r1cs_commit(ctx: *mut lh_ctx, srs: *const lh_srs, num_vars: usize, dim_vars: usize, m: *const lh_r1cs_matrix,
                          out: *mut *mut lh_r1cs_key) -> lh_status;
    // out null: the length alone; else *len is the room in and the length out
    pub fn lh_r1cs_commitment(key: *const lh_r1cs_key, out: *mut u8, len: *mut usize) -> lh_status;
    // d_w: 2^(dim_vars - 1) device elements; x: num_public host elements; the proof is appended to t
    pub fn lh_spartan_prove(ctx: *mut lh_ctx, srs: *const lh_srs, key: *const lh_r1cs_key, d_w: *const Fr, x: *const Fr,
                            num_public: usize, t: *mut lh_transcript) -> lh_status;
    pub fn lh_r1cs_free(ctx: *mut lh_ctx, key: *mut lh_r1cs_key);
    pub fn lh_spartan_verify(vp: *const lh_mkzg_vp, num_vars: usize, dim_vars: usize, commitment: *const u8,
                             commitment_len: usize, x: *const Fr, num_public: usize, t: *mut lh_transcript) -> lh_status;
    // (development) the keyed field sum alone: direction 0 by rows, 1 by columns; d_out: three device tables of 2^dim_vars
    pub fn lh_debug_spartan_spmv(ctx: *mut lh_ctx, key: *const lh_r1cs_key, direction: c_int, d_x: *const Fr,
                                 d_out: *const *mut Fr) -> lh_status;
    // Nova folding over an R1CS key (tests/nova_ref.py).  An instance blob is at most 160 + 32 num_public bytes; an entry that
    // makes one writes it to out_instance (*out_len: the room in, the length out).  d_e1 / d_e2 / d_e null: zero
    pub fn lh_nova_instance(ctx: *mut lh_ctx, srs: *const lh_srs, key: *const lh_r1cs_key, d_w: *const Fr, x: *const Fr,
                            num_public: usize, out_instance: *mut u8, out_len: *mut usize) -> lh_status;
    pub fn lh_nova_fold(ctx: *mut lh_ctx, srs: *const lh_srs, key: *const lh_r1cs_key, instance1: *const u8, instance1_len: usize,
                        instance2: *const u8, instance2_len: usize, d_w1: *const Fr, d_e1: *const Fr, d_w2: *const Fr,
                        d_e2: *const Fr, d_w_out: *mut Fr, d_e_out: *mut Fr, out_instance: *mut u8, out_len: *mut usize,
                        t: *mut lh_transcript) -> lh_status;
    pub fn lh_spartan_prove_relaxed(ctx: *mut lh_ctx, srs: *const lh_srs, key: *const lh_r1cs_key, instance: *const u8,
                                    instance_len: usize, d_w: *const Fr, d_e: *const Fr, t: *mut lh_transcript) -> lh_status;
    pub fn lh_nova_fold_verify(num_vars: usize, dim_vars: usize, commitment: *const u8, commitment_len: usize, instance1: *const u8,
                               instance1_len: usize, instance2: *const u8, instance2_len: usize, out_instance: *mut u8,
                               out_len: *mut usize, t: *mut lh_transcript) -> lh_status;
    pub fn lh_spartan_verify_relaxed(vp: *const lh_mkzg_vp, num_vars: usize, dim_vars: usize, commitment: *const u8,
                                     commitment_len: usize, instance: *const u8, instance_len: usize, num_public: usize,
                                     t: *mut lh_transcript) -> lh_status;
    // (development) the kernels of a fold alone
    pub fn lh_debug_nova_spmv2(ctx: *mut lh_ctx, key: *const lh_r1cs_key, direction: c_int, d_x1: *const Fr, d_x2: *const Fr,
                               d_out1: *const *mut Fr, d_out2: *const *mut Fr) -> lh_status;
    pub fn lh_debug_nova_cross_term(ctx: *mut lh_ctx, dim_vars: usize, d_mz1: *const *const Fr, d_mz2: *const *const Fr,
                                    d_e1: *const Fr, d_e2: *const Fr, u1: *const Fr, u2: *const Fr, d_t: *mut Fr,
                                    out_bad: *mut usize) -> lh_status;
    pub fn lh_debug_nova_fold(ctx: *mut lh_ctx, dim_vars: usize, d_w1: *const Fr, d_w2: *const Fr, d_w_out: *mut Fr, d_e1: *const Fr,
                              d_t: *const Fr, d_e2: *const Fr, d_e_out: *mut Fr, r: *const Fr) -> lh_status;
    // Batched Spartan, the verifier (tests/spartan_batch_ref.py): num_instances >= 2 assignments of one key in one proof; x:
    // num_instances * num_public elements, instance by instance
    pub fn lh_spartan_verify_batch(vp: *const lh_mkzg_vp, num_vars: usize, dim_vars: usize, commitment: *const u8,
                                   commitment_len: usize, x: *const Fr, num_instances: usize, num_public: usize,
                                   t: *mut lh_transcript) -> lh_status;
    // the host verifier of lh_gkr_fractional_prove; the roots p_0s / q_0s come back with the final claims and the point
    pub fn lh_gkr_fractional_verify(num_batching: usize, num_vars: usize, claimed_p_0s: *const *const Fr,
                                    claimed_q_0s: *const *const Fr, t: *mut lh_transcript, out_p_0s: *mut Fr,
                                    out_q_0s: *mut Fr, out_p_xs: *mut Fr, out_q_xs: *mut Fr, out_x: *mut Fr) -> lh_status;
    // one proof over several GPUs
    pub fn lh_ctx_set_comm(ctx: *mut lh_ctx, comm: *const lh_comm, shard_bit: usize) -> lh_status;
    pub fn lh_rccl_unique_id(out: *mut u8) -> lh_status;
    pub fn lh_ctx_set_comm_rccl(ctx: *mut lh_ctx, rank: c_int, size: c_int, unique_id: *const u8, shard_bit: usize) -> lh_status;
    pub fn lh_ctx_set_comm_loopback(ctx: *mut lh_ctx, rank: c_int, size: c_int, shard_bit: usize) -> lh_status;
    pub fn lh_ctx_comm_stats(ctx: *mut lh_ctx, out: *mut u64) -> lh_status;
    pub fn lh_ctx_comm_phase_stats(ctx: *mut lh_ctx, out: *mut u64, reset: c_int) -> lh_status;
    pub fn lh_ctx_memory_stats(ctx: *mut lh_ctx, out: *mut u64) -> lh_status;
    pub fn lh_ctx_compute_units(ctx: *mut lh_ctx, out: *mut usize) -> lh_status;
    pub fn lh_ctx_host_cpus(ctx: *mut lh_ctx, bus_id: *mut c_char, bus_id_cap: usize, cpulist: *mut c_char, cpulist_cap: usize) -> lh_status;
    pub fn lh_shard_extract(ctx: *mut lh_ctx, d_global: *const c_void, n_local: usize, shard_bit: usize, rho: usize,
                            rank: usize, elem_bytes: usize, d_local: *mut c_void) -> lh_status;
    // route options (include/lasso_hip.h lists the names) and the route the last Lasso prove took
    pub fn lh_ctx_set_option(ctx: *mut lh_ctx, name: *const c_char, value: i64) -> lh_status;
    pub fn lh_ctx_get_option(ctx: *mut lh_ctx, name: *const c_char, out: *mut i64) -> lh_status;
    pub fn lh_lasso_last_route(ctx: *mut lh_ctx, out: *mut lh_lasso_route) -> lh_status;
    // caller-registered subtables: host only, no ctx (lasso.rs Subtable)
    pub fn lh_subtable_register(values: *const u32, chunk_bits: u32, out_kind: *mut u32) -> lh_status;
    pub fn lh_subtable_unregister(kind: u32) -> lh_status;
    pub fn lh_subtable_info(kind: u32, chunk_bits: *mut u32, value_bits: *mut u32, digest32: *mut u8) -> lh_status;
    pub fn lh_lasso_prove_sharded(ctx: *mut lh_ctx, srs: *const lh_srs, table: *const lh_lasso_table, num_vars: usize,
                                  d_dims_local: *const *const u32, t: *mut lh_transcript) -> lh_status;
    // HyperPlonk
    pub fn lh_hyperplonk_prove(ctx: *mut lh_ctx, srs: *const lh_srs, pp: *const lh_hp_param,
                               instances: *const *const Fr, d_witness_polys: *const *const Fr,
                               t: *mut lh_transcript) -> lh_status;
    pub fn lh_hyperplonk_prove_sharded(ctx: *mut lh_ctx, srs: *const lh_srs, pp: *const lh_hp_param,
                                       instances: *const *const Fr, d_witness_polys_local: *const *const Fr,
                                       t: *mut lh_transcript) -> lh_status;
    pub fn lh_hyperplonk_prove_phases(ctx: *mut lh_ctx, srs: *const lh_srs, pp: *const lh_hp_param, num_phases: usize,
                                      num_witness_polys: *const usize, num_challenges: *const usize,
                                      instances: *const *const Fr, circuit: *const lh_hp_circuit,
                                      t: *mut lh_transcript) -> lh_status;
    pub fn lh_hyperplonk_verify(vp: *const lh_mkzg_vp, hvp: *const lh_hp_vparam, instances: *const *const Fr,
                                t: *mut lh_transcript) -> lh_status;
    pub fn lh_hyperplonk_verify_phases(vp: *const lh_mkzg_vp, hvp: *const lh_hp_vparam, num_phases: usize,
                                       num_witness_polys: *const usize, num_challenges: *const usize,
                                       instances: *const *const Fr, t: *mut lh_transcript) -> lh_status;
    // multi-phase circuits over Zeromorph (hyperplonk.rs:185-205 is PCS-generic; lh_usrs / lh_zm_vp are opaque here)
    pub fn lh_hyperplonk_prove_phases_zeromorph(ctx: *mut lh_ctx, srs: *const core::ffi::c_void, poly_size: usize,
                                                pp: *const lh_hp_param, num_phases: usize,
                                                num_witness_polys: *const usize, num_challenges: *const usize,
                                                instances: *const *const Fr, circuit: *const lh_hp_circuit,
                                                t: *mut lh_transcript) -> lh_status;
    pub fn lh_hyperplonk_verify_phases_zeromorph(vp: *const core::ffi::c_void, hvp: *const lh_hp_vparam, num_phases: usize,
                                                 num_witness_polys: *const usize, num_challenges: *const usize,
                                                 instances: *const *const Fr, t: *mut lh_transcript) -> lh_status;
    // (development) the source text of a runtime-compiled round kernel
    pub fn lh_debug_jit_source(code: *const u32, num_instrs: usize, num_regs: u32, result_reg: u32, degree: i32,
                               out: *mut core::ffi::c_char, cap: usize, len: *mut usize) -> lh_status;
    // (development) the radix sort and the Lasso access counters on their own; lh_debug_sort_plan is host only
    pub fn lh_debug_sort_pairs(ctx: *mut lh_ctx, key_bytes: i32, slabs: *const lh_debug_sort_slab, count: usize) -> lh_status;
    pub fn lh_debug_lasso_counters(ctx: *mut lh_ctx, d_dims: *const *const u32, num_cols: usize, n: usize, m: usize,
                                   d_read_ts: *const *mut u32, d_final_cts: *const *mut u32,
                                   d_keep_sorted: *const *mut u32, d_keep_index: *const *mut u32) -> lh_status;
    pub fn lh_debug_sort_plan(n: usize, bits: u32, key_bytes: i32, passes: *mut u32, rb: *mut u32,
                              temp_bytes: *mut usize) -> lh_status;
    // (development) the owners of device resources: live counts (device blocks, pinned blocks, events, streams) and a
    // one-shot failure of the (n + 1)-th acquisition from now on (n < 0: off); host only
    pub fn lh_debug_live_resources(out: *mut u64) -> lh_status;
    pub fn lh_debug_fail_acquire_after(n: i64) -> lh_status;
    // (development) the 32-bit column kernels on their own
    pub fn lh_debug_u32_columns(ctx: *mut lh_ctx, op: i32, args: *const lh_debug_u32_args) -> lh_status;
    // (development) the Lasso witness's subtable read for one memory, built-in or registered kind
    pub fn lh_debug_lasso_subtable_read(ctx: *mut lh_ctx, kind: u32, chunk_bits: u32, d_dim: *const u32, n: usize,
                                        d_out: *mut u32) -> lh_status;
    // Zeromorph over univariate KZG: lh_ukzg_setup, lh_usrs_*, lh_zeromorph_* follow the same shapes
    // (include/lasso_hip.h, section f3) and are bound the same way when HyperPlonk<Zeromorph<..>> is wanted.
    // Univariate KZG on its own and Gemini over it (include/lasso_hip.h, section f3b); lh_usrs / lh_ukzg_vp are opaque here
    pub fn lh_ukzg_batch_commit(ctx: *mut lh_ctx, srs: *const c_void, poly_size: usize, d_polys: *const *const Fr,
                                lens: *const usize, num_polys: usize, out_comms: *mut G1Affine) -> lh_status;
    pub fn lh_ukzg_open(ctx: *mut lh_ctx, srs: *const c_void, poly_size: usize, d_poly: *const Fr, len: usize,
                        point: *const Fr, t: *mut lh_transcript) -> lh_status;
    pub fn lh_ukzg_batch_open(ctx: *mut lh_ctx, srs: *const c_void, poly_size: usize, d_polys: *const *const Fr,
                              lens: *const usize, num_polys: usize, points: *const Fr, num_points: usize,
                              evals: *const lh_evaluation, num_evals: usize, t: *mut lh_transcript) -> lh_status;
    pub fn lh_ukzg_vp_setup(s: *const Fr, out: *mut *mut c_void) -> lh_status;
    pub fn lh_ukzg_vp_free(vp: *mut c_void);
    pub fn lh_ukzg_verify(vp: *const c_void, comm: *const G1Affine, point: *const Fr, eval: *const Fr,
                          t: *mut lh_transcript) -> lh_status;
    pub fn lh_ukzg_batch_verify(vp: *const c_void, comms: *const G1Affine, num_comms: usize, points: *const Fr,
                                num_points: usize, evals: *const lh_evaluation, num_evals: usize,
                                t: *mut lh_transcript) -> lh_status;
    pub fn lh_gemini_batch_commit(ctx: *mut lh_ctx, srs: *const c_void, poly_size: usize, d_polys: *const *const Fr,
                                  num_polys: usize, num_vars: usize, out_comms: *mut G1Affine) -> lh_status;
    pub fn lh_gemini_open(ctx: *mut lh_ctx, srs: *const c_void, poly_size: usize, d_poly: *const Fr, num_vars: usize,
                          point: *const Fr, t: *mut lh_transcript) -> lh_status;
    pub fn lh_gemini_batch_open(ctx: *mut lh_ctx, srs: *const c_void, poly_size: usize, num_vars: usize,
                                d_polys: *const *const Fr, num_polys: usize, points: *const Fr, num_points: usize,
                                evals: *const lh_evaluation, num_evals: usize, t: *mut lh_transcript) -> lh_status;
    pub fn lh_gemini_verify(vp: *const c_void, comm: *const G1Affine, point: *const Fr, num_vars: usize, eval: *const Fr,
                            t: *mut lh_transcript) -> lh_status;
    pub fn lh_gemini_batch_verify(vp: *const c_void, num_vars: usize, comms: *const G1Affine, num_comms: usize,
                                  points: *const Fr, num_points: usize, evals: *const lh_evaluation, num_evals: usize,
                                  t: *mut lh_transcript) -> lh_status;
    pub fn lh_lasso_prove_gemini(ctx: *mut lh_ctx, srs: *const c_void, poly_size: usize, table: *const lh_lasso_table,
                                 num_vars: usize, d_dims: *const *const u32, t: *mut lh_transcript) -> lh_status;
    pub fn lh_lasso_verify_gemini(vp: *const c_void, table: *const lh_lasso_table, num_vars: usize,
                                  t: *mut lh_transcript) -> lh_status;
    pub fn lh_hyperplonk_prove_gemini(ctx: *mut lh_ctx, srs: *const c_void, poly_size: usize, pp: *const lh_hp_param,
                                      instances: *const *const Fr, d_witness_polys: *const *const Fr,
                                      t: *mut lh_transcript) -> lh_status;
    pub fn lh_hyperplonk_verify_gemini(vp: *const c_void, hvp: *const lh_hp_vparam, instances: *const *const Fr,
                                       t: *mut lh_transcript) -> lh_status;
    // The multilinear IPA over bn256::G1Affine (include/lasso_hip.h, section f5); lh_ipa_param is opaque here
    pub fn lh_ipa_setup(ctx: *mut lh_ctx, poly_size: usize, out: *mut *mut c_void) -> lh_status;
    pub fn lh_ipa_param_free(ctx: *mut lh_ctx, param: *mut c_void);
    pub fn lh_ipa_param_size(param: *const c_void) -> usize;
    pub fn lh_ipa_param_download(ctx: *mut lh_ctx, param: *const c_void, g: *mut G1Affine, h: *mut G1Affine) -> lh_status;
    pub fn lh_ipa_batch_commit(ctx: *mut lh_ctx, param: *const c_void, poly_size: usize, d_polys: *const *const Fr,
                               num_polys: usize, num_vars: usize, out_comms: *mut G1Affine) -> lh_status;
    pub fn lh_ipa_open(ctx: *mut lh_ctx, param: *const c_void, poly_size: usize, d_poly: *const Fr, num_vars: usize,
                       point: *const Fr, t: *mut lh_transcript) -> lh_status;
    pub fn lh_ipa_batch_open(ctx: *mut lh_ctx, param: *const c_void, poly_size: usize, num_vars: usize,
                             d_polys: *const *const Fr, num_polys: usize, points: *const Fr, num_points: usize,
                             evals: *const lh_evaluation, num_evals: usize, t: *mut lh_transcript) -> lh_status;
    pub fn lh_ipa_verify(param: *const c_void, poly_size: usize, comm: *const G1Affine, point: *const Fr, num_vars: usize,
                         eval: *const Fr, t: *mut lh_transcript) -> lh_status;
    pub fn lh_ipa_batch_verify(param: *const c_void, poly_size: usize, num_vars: usize, comms: *const G1Affine,
                               num_comms: usize, points: *const Fr, num_points: usize, evals: *const lh_evaluation,
                               num_evals: usize, t: *mut lh_transcript) -> lh_status;
    pub fn lh_g1_axpy(ctx: *mut lh_ctx, d_a: *const G1Affine, d_b: *const G1Affine, n: usize, s: *const Fr,
                      d_out: *mut G1Affine) -> lh_status;
    pub fn lh_g1_rows_msm(ctx: *mut lh_ctx, d_scalars: *const c_void, scalars_u32: c_int, bits: u32, n: usize, row_len: usize,
                          d_bases: *const G1Affine, out_rows: *mut G1Affine) -> lh_status;
    pub fn lh_lasso_prove_hyrax(ctx: *mut lh_ctx, param: *const c_void, poly_size: usize, batch_size: usize,
                                table: *const lh_lasso_table, num_vars: usize, d_dims: *const *const u32,
                                t: *mut lh_transcript) -> lh_status;
    pub fn lh_lasso_verify_hyrax(param: *const c_void, poly_size: usize, batch_size: usize, table: *const lh_lasso_table,
                                 num_vars: usize, t: *mut lh_transcript) -> lh_status;
    pub fn lh_hyperplonk_prove_hyrax(ctx: *mut lh_ctx, param: *const c_void, poly_size: usize, batch_size: usize,
                                     pp: *const lh_hp_param, instances: *const *const Fr, d_witness_polys: *const *const Fr,
                                     t: *mut lh_transcript) -> lh_status;
    pub fn lh_hyperplonk_verify_hyrax(param: *const c_void, poly_size: usize, batch_size: usize, hvp: *const lh_hp_vparam,
                                      instances: *const *const Fr, t: *mut lh_transcript) -> lh_status;
    pub fn lh_hyperplonk_prove_phases_hyrax(ctx: *mut lh_ctx, param: *const c_void, poly_size: usize, batch_size: usize,
                                            pp: *const lh_hp_param, num_phases: usize, num_witness_polys: *const usize,
                                            num_challenges: *const usize, instances: *const *const Fr,
                                            circuit: *const lh_hp_circuit, t: *mut lh_transcript) -> lh_status;
    pub fn lh_hyperplonk_verify_phases_hyrax(param: *const c_void, poly_size: usize, batch_size: usize,
                                             hvp: *const lh_hp_vparam, num_phases: usize, num_witness_polys: *const usize,
                                             num_challenges: *const usize, instances: *const *const Fr,
                                             t: *mut lh_transcript) -> lh_status;
    pub fn lh_lasso_prove_ipa(ctx: *mut lh_ctx, param: *const c_void, poly_size: usize, table: *const lh_lasso_table,
                              num_vars: usize, d_dims: *const *const u32, t: *mut lh_transcript) -> lh_status;
    pub fn lh_lasso_verify_ipa(param: *const c_void, poly_size: usize, table: *const lh_lasso_table, num_vars: usize,
                               t: *mut lh_transcript) -> lh_status;
    pub fn lh_hyperplonk_prove_ipa(ctx: *mut lh_ctx, param: *const c_void, poly_size: usize, pp: *const lh_hp_param,
                                   instances: *const *const Fr, d_witness_polys: *const *const Fr,
                                   t: *mut lh_transcript) -> lh_status;
    pub fn lh_hyperplonk_verify_ipa(param: *const c_void, poly_size: usize, hvp: *const lh_hp_vparam,
                                    instances: *const *const Fr, t: *mut lh_transcript) -> lh_status;
    pub fn lh_hyperplonk_prove_phases_ipa(ctx: *mut lh_ctx, param: *const c_void, poly_size: usize, pp: *const lh_hp_param,
                                          num_phases: usize, num_witness_polys: *const usize, num_challenges: *const usize,
                                          instances: *const *const Fr, circuit: *const lh_hp_circuit,
                                          t: *mut lh_transcript) -> lh_status;
    pub fn lh_hyperplonk_verify_phases_ipa(param: *const c_void, poly_size: usize, hvp: *const lh_hp_vparam, num_phases: usize,
                                           num_witness_polys: *const usize, num_challenges: *const usize,
                                           instances: *const *const Fr, t: *mut lh_transcript) -> lh_status;
    // Hyrax on top of the IPA (same section); its param is an lh_ipa_param
    pub fn lh_hyrax_setup(ctx: *mut lh_ctx, poly_size: usize, batch_size: usize, out: *mut *mut c_void) -> lh_status;
    pub fn lh_hyrax_dims(poly_size: usize, batch_size: usize, num_vars: *mut usize, batch_num_vars: *mut usize,
                         row_num_vars: *mut usize) -> lh_status;
    pub fn lh_hyrax_trim(param: *const c_void, poly_size: usize, batch_size: usize, row_num_vars: *mut usize,
                         num_chunks: *mut usize) -> lh_status;
    pub fn lh_hyrax_batch_commit(ctx: *mut lh_ctx, param: *const c_void, poly_size: usize, batch_size: usize,
                                 d_polys: *const *const Fr, num_polys: usize, num_vars: usize, out_comms: *mut G1Affine) -> lh_status;
    pub fn lh_hyrax_open(ctx: *mut lh_ctx, param: *const c_void, poly_size: usize, batch_size: usize, d_poly: *const Fr,
                         num_vars: usize, point: *const Fr, t: *mut lh_transcript) -> lh_status;
    pub fn lh_hyrax_batch_open(ctx: *mut lh_ctx, param: *const c_void, poly_size: usize, batch_size: usize, num_vars: usize,
                               d_polys: *const *const Fr, num_polys: usize, points: *const Fr, num_points: usize,
                               evals: *const lh_evaluation, num_evals: usize, t: *mut lh_transcript) -> lh_status;
    pub fn lh_hyrax_verify(param: *const c_void, poly_size: usize, batch_size: usize, comm: *const G1Affine, point: *const Fr,
                           num_vars: usize, eval: *const Fr, t: *mut lh_transcript) -> lh_status;
    pub fn lh_hyrax_batch_verify(param: *const c_void, poly_size: usize, batch_size: usize, num_vars: usize,
                                 comms: *const G1Affine, num_comms: usize, points: *const Fr, num_points: usize,
                                 evals: *const lh_evaluation, num_evals: usize, t: *mut lh_transcript) -> lh_status;
    // Brakedown (include/lasso_hip.h, section f4); params and commitments are opaque here
    pub fn lh_keccak_transcript_hash_io(t: *mut lh_transcript, out: *mut lh_hash_transcript) -> lh_status;
    pub fn lh_brakedown_setup(ctx: *mut lh_ctx, num_vars: usize, spec: c_int, seed32: *const u8,
                              out: *mut *mut c_void) -> lh_status;
    pub fn lh_brakedown_derive(num_vars: usize, spec: c_int, out: *mut *mut c_void) -> lh_status;
    // Ligero (section f4b): the same scheme over Reed-Solomon rows; `row_vars` usize::MAX chooses the row length
    pub fn lh_ligero_setup(ctx: *mut lh_ctx, num_vars: usize, log_inv_rate: c_int, row_vars: usize,
                           out: *mut *mut c_void) -> lh_status;
    pub fn lh_ligero_derive(num_vars: usize, log_inv_rate: c_int, row_vars: usize, out: *mut *mut c_void) -> lh_status;
    pub fn lh_brakedown_param_info(pp: *const c_void, row_len: *mut usize, num_rows: *mut usize,
                                   codeword_len: *mut usize, num_column_opening: *mut usize,
                                   num_proximity_testing: *mut usize) -> lh_status;
    pub fn lh_brakedown_trim(pp: *const c_void, poly_size: usize) -> lh_status;
    pub fn lh_brakedown_param_free(pp: *mut c_void);
    pub fn lh_brakedown_encode(pp: *const c_void, msg: *const Fr, out: *mut Fr) -> lh_status;
    pub fn lh_brakedown_commit(ctx: *mut lh_ctx, pp: *const c_void, d_poly: *const Fr, num_vars: usize,
                               out: *mut *mut c_void) -> lh_status;
    pub fn lh_brakedown_batch_commit(ctx: *mut lh_ctx, pp: *const c_void, d_polys: *const *const Fr, num_polys: usize,
                                     num_vars: usize, out: *mut *mut c_void) -> lh_status;
    /// kinds: 0 = Fr (Montgomery), 1 = u32; column i is lens[i] <= 2^num_vars entries, committed zero-padded
    pub fn lh_brakedown_commit_columns(ctx: *mut lh_ctx, pp: *const c_void, d_cols: *const *const c_void, kinds: *const c_int,
                                       lens: *const usize, num_cols: usize, out: *mut *mut c_void) -> lh_status;
    pub fn lh_brakedown_comm_root(comm: *const c_void, out32: *mut u8) -> lh_status;
    pub fn lh_brakedown_comm_rows(ctx: *mut lh_ctx, comm: *const c_void, out: *mut Fr) -> lh_status;
    pub fn lh_brakedown_comm_rows_device(comm: *const c_void, d_out: *mut *mut Fr) -> lh_status;
    pub fn lh_brakedown_comm_free(comm: *mut c_void);
    pub fn lh_brakedown_open(ctx: *mut lh_ctx, pp: *const c_void, d_poly: *const Fr, num_vars: usize, comm: *mut c_void,
                             point: *const Fr, t: *mut lh_transcript, ht: *mut lh_hash_transcript) -> lh_status;
    pub fn lh_brakedown_batch_open(ctx: *mut lh_ctx, pp: *const c_void, num_vars: usize, d_polys: *const *const Fr,
                                   comms: *const *mut c_void, num_polys: usize, points: *const Fr, num_points: usize,
                                   evals: *const lh_evaluation, num_evals: usize, t: *mut lh_transcript,
                                   ht: *mut lh_hash_transcript) -> lh_status;
    pub fn lh_brakedown_read_commitments(pp: *const c_void, num: usize, ht: *mut lh_hash_transcript,
                                         out: *mut u8) -> lh_status;
    pub fn lh_brakedown_verify(pp: *const c_void, root32: *const u8, point: *const Fr, num_vars: usize,
                               eval: *const Fr, t: *mut lh_transcript, ht: *mut lh_hash_transcript) -> lh_status;
    pub fn lh_brakedown_batch_verify(pp: *const c_void, num_vars: usize, roots: *const u8, num_comms: usize,
                                     points: *const Fr, num_points: usize, evals: *const lh_evaluation,
                                     num_evals: usize, t: *mut lh_transcript, ht: *mut lh_hash_transcript) -> lh_status;
    pub fn lh_brakedown_comm_tree(ctx: *mut lh_ctx, comm: *const c_void, out: *mut u8) -> lh_status;
    pub fn lh_brakedown_comm_stage(ctx: *mut lh_ctx, pp: *const c_void, comm: *const c_void, out: *mut Fr) -> lh_status;
    // HyperPlonk over Brakedown: the commitments of the preprocess and permutation polys on the prove side, their roots
    // (32 bytes each) on the verify side; hvp's two point arrays are ignored
    pub fn lh_hyperplonk_prove_brakedown(ctx: *mut lh_ctx, param: *const c_void, pp: *const lh_hp_param,
                                         preprocess_comms: *const *mut c_void, permutation_comms: *const *mut c_void,
                                         instances: *const *const Fr, d_witness_polys: *const *const Fr,
                                         t: *mut lh_transcript, ht: *mut lh_hash_transcript) -> lh_status;
    pub fn lh_hyperplonk_prove_phases_brakedown(ctx: *mut lh_ctx, param: *const c_void, pp: *const lh_hp_param,
                                                preprocess_comms: *const *mut c_void, permutation_comms: *const *mut c_void,
                                                num_phases: usize, num_witness_polys: *const usize,
                                                num_challenges: *const usize, instances: *const *const Fr,
                                                circuit: *const lh_hp_circuit, t: *mut lh_transcript,
                                                ht: *mut lh_hash_transcript) -> lh_status;
    pub fn lh_hyperplonk_verify_brakedown(param: *const c_void, hvp: *const lh_hp_vparam, preprocess_roots: *const u8,
                                          permutation_roots: *const u8, instances: *const *const Fr, t: *mut lh_transcript,
                                          ht: *mut lh_hash_transcript) -> lh_status;
    pub fn lh_hyperplonk_verify_phases_brakedown(param: *const c_void, hvp: *const lh_hp_vparam, preprocess_roots: *const u8,
                                                 permutation_roots: *const u8, num_phases: usize,
                                                 num_witness_polys: *const usize, num_challenges: *const usize,
                                                 instances: *const *const Fr, t: *mut lh_transcript,
                                                 ht: *mut lh_hash_transcript) -> lh_status;
    pub fn lh_lasso_prove_brakedown(ctx: *mut lh_ctx, param: *const c_void, table: *const lh_lasso_table, num_vars: usize,
                                    d_dims: *const *const u32, t: *mut lh_transcript, ht: *mut lh_hash_transcript) -> lh_status;
    pub fn lh_lasso_verify_brakedown(param: *const c_void, table: *const lh_lasso_table, num_vars: usize, t: *mut lh_transcript,
                                     ht: *mut lh_hash_transcript) -> lh_status;
}
