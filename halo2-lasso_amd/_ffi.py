"""ctypes binding of liblasso_hip.so -- the declarations of include/lasso_hip.h.

Loading fails loudly when the library has not been built (`__graft_entry__.build()` or
`make -C halo2-lasso_amd/csrc`): there is no Python or CPU fallback for any compute call.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liblasso_hip.so")

LH_OK = 0
LH_ERR_INVALID_SUMCHECK, LH_ERR_INVALID_PCS_PARAM, LH_ERR_INVALID_PCS_OPEN = -1, -2, -3
LH_ERR_INVALID_SNARK, LH_ERR_SERIALIZATION, LH_ERR_TRANSCRIPT, LH_ERR_DEVICE, LH_ERR_ARG = -4, -5, -6, -7, -8
LH_SC_EVALUATIONS, LH_SC_COEFFICIENTS = 0, 1
LH_SC_MAX_TERMS, LH_SC_MAX_FACTORS = 48, 4
LH_LASSO_MAX_CHUNKS, LH_LASSO_MAX_MEMORIES, LH_LASSO_MAX_TERMS = 8, 16, 16
LH_SUBTABLE_IDENTITY, LH_SUBTABLE_AND, LH_SUBTABLE_XOR, LH_SUBTABLE_OR, LH_SUBTABLE_EQ, LH_SUBTABLE_LTU = 0, 1, 2, 3, 4, 5
LH_SUBTABLE_CUSTOM_BASE, LH_SUBTABLE_CUSTOM_MAX, LH_SUBTABLE_CUSTOM_MAX_BITS = 0x100, 64, 20  # lh_subtable_register
LH_LASSO_NUM_PHASES = 9
LH_LOGUP_MAX_LOOKUPS, LH_LOGUP_MAX_WIDTH, LH_LOGUP_MAX_TABLE_VARS = 8, 8, 24  # lh_logup_gkr_prove
LH_LOGUP_COL_FR, LH_LOGUP_COL_U32 = 0, 1  # lh_logup_columns.kinds
LH_MEMCHECK_MAX_INIT_VARS = 24  # lh_memcheck_prove: mem_vars with an initial image
LH_SPARK_MAX_DIMS, LH_SPARK_MAX_DIM_VARS = 3, 24  # lh_spark_commit
LH_SPARTAN_MIN_DIM_VARS, LH_SPARTAN_MAX_DIM_VARS = 2, 24  # lh_r1cs_commit
LH_SPARTAN_BATCH_MAX_VARS = 26  # lh_spartan_verify_batch: dim_vars + batch_vars
LH_BD_COLUMN_FR, LH_BD_COLUMN_U32 = 0, 1
LH_LIGERO_ROW_VARS_AUTO = (1 << 64) - 1  # (size_t)-1


class lh_fr(C.Structure):
    _fields_ = [("l", C.c_uint64 * 4)]


class lh_g1(C.Structure):
    _fields_ = [("x", C.c_uint64 * 4), ("y", C.c_uint64 * 4)]


class lh_sop(C.Structure):
    _fields_ = [("num_terms", C.c_uint32), ("global_eq", C.c_int32),
                ("coeff", lh_fr * LH_SC_MAX_TERMS),
                ("num_factors", C.c_uint8 * LH_SC_MAX_TERMS),
                ("factor", (C.c_uint8 * LH_SC_MAX_FACTORS) * LH_SC_MAX_TERMS)]


class lh_expr_node(C.Structure):
    _fields_ = [("op", C.c_uint32), ("a", C.c_int32), ("b", C.c_int32), ("reserved", C.c_uint32), ("scalar", lh_fr)]


class lh_expr(C.Structure):
    _fields_ = [("nodes", C.POINTER(lh_expr_node)), ("num_nodes", C.c_size_t)]


class lh_lasso_table(C.Structure):
    _fields_ = [("num_chunks", C.c_uint32), ("chunk_bits", C.c_uint32), ("num_memories", C.c_uint32),
                ("memory_chunk", C.c_uint32 * LH_LASSO_MAX_MEMORIES),
                ("memory_subtable", C.c_uint32 * LH_LASSO_MAX_MEMORIES),
                ("num_terms", C.c_uint32),
                ("g_coeff", lh_fr * LH_LASSO_MAX_TERMS),
                ("g_num_factors", C.c_uint8 * LH_LASSO_MAX_TERMS),
                ("g_factor", (C.c_uint8 * LH_SC_MAX_FACTORS) * LH_LASSO_MAX_TERMS)]


class lh_logup_lookup(C.Structure):
    _fields_ = [("width", C.c_uint32), ("d_inputs", C.POINTER(C.c_void_p)), ("table", C.POINTER(C.POINTER(lh_fr)))]


class lh_memcheck_trace(C.Structure):
    _fields_ = [("d_addr", C.POINTER(C.c_uint32)), ("d_rv", C.POINTER(C.c_uint32)), ("d_wv", C.POINTER(C.c_uint32))]


class lh_memcheck_ops(C.Structure):
    _fields_ = [("d_addr", C.POINTER(C.c_uint32)), ("d_store", C.POINTER(C.c_uint32)), ("d_val", C.POINTER(C.c_uint32))]


class lh_r1cs_matrix(C.Structure):
    _fields_ = [("d_row", C.POINTER(C.c_uint32)), ("d_col", C.POINTER(C.c_uint32)), ("d_val", C.POINTER(lh_fr))]


class lh_logup_columns(C.Structure):
    _fields_ = [("width", C.c_uint32), ("d_inputs", C.POINTER(C.c_void_p)), ("kinds", C.POINTER(C.c_uint8)),
                ("table", C.POINTER(C.POINTER(lh_fr)))]


class lh_hp_lasso_lookup(C.Structure):
    _fields_ = [("table", lh_lasso_table), ("output_poly", C.c_size_t), ("chunk_polys", C.c_size_t * LH_LASSO_MAX_CHUNKS)]


class lh_hp_lookup(C.Structure):
    _fields_ = [("inputs", C.POINTER(lh_expr)), ("tables", C.POINTER(lh_expr)), ("width", C.c_size_t)]


class lh_hp_param(C.Structure):
    _fields_ = [("num_vars", C.c_size_t),
                ("num_instance_polys", C.c_size_t), ("num_instances", C.POINTER(C.c_size_t)),
                ("num_preprocess_polys", C.c_size_t), ("d_preprocess_polys", C.POINTER(C.c_void_p)),
                ("num_witness_polys", C.c_size_t), ("num_challenges", C.c_size_t),
                ("num_lookups", C.c_size_t), ("lookups", C.POINTER(lh_hp_lookup)),
                ("num_permutation_polys", C.c_size_t), ("permutation_poly_index", C.POINTER(C.c_size_t)),
                ("d_permutation_polys", C.POINTER(C.c_void_p)),
                ("num_permutation_z_polys", C.c_size_t),
                ("expression", lh_expr),
                ("num_lasso_lookups", C.c_size_t), ("lasso_lookups", C.POINTER(lh_hp_lasso_lookup))]


_SYNTH_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_size_t, C.POINTER(lh_fr), C.c_size_t, C.POINTER(C.c_void_p), C.c_size_t)


class lh_hp_circuit(C.Structure):
    _fields_ = [("user", C.c_void_p), ("synthesize", _SYNTH_CB)]


class lh_hp_vparam(C.Structure):
    _fields_ = [("num_vars", C.c_size_t),
                ("num_instance_polys", C.c_size_t), ("num_instances", C.POINTER(C.c_size_t)),
                ("num_witness_polys", C.c_size_t), ("num_challenges", C.c_size_t),
                ("num_lookups", C.c_size_t), ("num_permutation_z_polys", C.c_size_t),
                ("expression", lh_expr),
                ("num_preprocess_polys", C.c_size_t), ("preprocess_comms", C.POINTER(lh_g1)),
                ("num_permutation_polys", C.c_size_t), ("permutation_comms", C.POINTER(lh_g1)),
                ("num_lasso_lookups", C.c_size_t), ("lasso_lookups", C.POINTER(lh_hp_lasso_lookup))]


class lh_evaluation(C.Structure):
    _fields_ = [("poly", C.c_uint32), ("point", C.c_uint32), ("value", lh_fr)]


_AG_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t)
_AGD_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)
LH_RCCL_UNIQUE_ID_BYTES = 128


class lh_comm(C.Structure):
    _fields_ = [("rank", C.c_int), ("size", C.c_int), ("user", C.c_void_p), ("all_gather", _AG_CB),
                ("all_gather_device", _AGD_CB)]


class lh_debug_sort_slab(C.Structure):  # (development: lh_debug_sort_pairs)
    _fields_ = [("d_keys_in", C.c_void_p), ("d_keys_out", C.c_void_p), ("d_vals_in", C.c_void_p), ("d_vals_out", C.c_void_p),
                ("n", C.c_size_t), ("bits", C.c_uint32), ("first_bit", C.c_uint32)]


class lh_debug_u32_args(C.Structure):  # (development: lh_debug_u32_columns)
    _fields_ = [("d_cols", C.POINTER(C.c_void_p)), ("lens", C.POINTER(C.c_size_t)), ("w", C.POINTER(lh_fr)),
                ("count", C.c_size_t), ("d_weights", C.c_void_p), ("n", C.c_size_t),
                ("d_fr", C.POINTER(C.c_void_p)), ("w_fr", C.POINTER(lh_fr)), ("num_fr", C.c_size_t),
                ("r0", lh_fr), ("r1", lh_fr), ("d_out", C.c_void_p), ("out_host", C.POINTER(lh_fr)),
                ("taken", C.POINTER(C.c_int))]


LH_U32_OPS = ("inner_products_small", "inner_products_small_half", "inner_products_small_quads", "inner_products_quads",
              "lincomb_mixed", "lincomb_fold_small", "lincomb_bind2", "sc_round_u32_bind2", None,
              "quad_sums")  # index = the op code (8 is not an operation)


class lh_prof_rec(C.Structure):
    _fields_ = [("name", C.c_char * 40), ("ms", C.c_double), ("bytes", C.c_double), ("muls", C.c_double),
                ("items", C.c_double)]


_FE_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(lh_fr))
_G1_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(lh_g1))


class lh_transcript(C.Structure):
    _fields_ = [("user", C.c_void_p),
                ("write_field_element", _FE_CB), ("common_field_element", _FE_CB),
                ("squeeze_challenge", _FE_CB),
                ("write_commitment", _G1_CB), ("common_commitment", _G1_CB),
                ("read_field_element", _FE_CB), ("read_commitment", _G1_CB)]


_HASH_W_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_uint8))


class lh_hash_transcript(C.Structure):
    _fields_ = [("user", C.c_void_p), ("write_hash", _HASH_W_CB), ("read_hash", _HASH_W_CB)]


class lh_g2(C.Structure):
    _fields_ = [("x_c0", C.c_uint64 * 4), ("x_c1", C.c_uint64 * 4), ("y_c0", C.c_uint64 * 4), ("y_c1", C.c_uint64 * 4)]


_P = C.c_void_p
_SZ = C.c_size_t
# name -> (restype, argtypes); every symbol include/lasso_hip.h declares (the Lasso / HyperPlonk entries of the point
# commitment schemes are added below the literal rows)
SIGNATURES = {
    "lh_last_error": (C.c_char_p, []),
    "lh_version": (C.c_char_p, []),
    "lh_ctx_create": (C.c_int, [C.c_int, C.POINTER(_P)]),
    "lh_ctx_destroy": (None, [_P]),
    "lh_ctx_sync": (C.c_int, [_P]),
    "lh_ctx_stream": (_P, [_P]),
    "lh_alloc": (C.c_int, [_P, _SZ, C.POINTER(_P)]),
    "lh_free": (C.c_int, [_P, _P]),
    "lh_upload": (C.c_int, [_P, _P, _P, _SZ]),
    "lh_download": (C.c_int, [_P, _P, _P, _SZ]),
    "lh_keccak_transcript_new": (C.c_int, [C.POINTER(C.POINTER(lh_transcript))]),
    "lh_keccak_transcript_free": (None, [C.POINTER(lh_transcript)]),
    "lh_keccak_transcript_proof": (C.c_int, [C.POINTER(lh_transcript), C.POINTER(C.POINTER(C.c_uint8)),
                                             C.POINTER(_SZ)]),
    "lh_fr_from_u64": (C.c_int, [_P, _P, _SZ, _P]),
    "lh_fr_from_u32": (C.c_int, [_P, _P, _SZ, _P]),
    "lh_fr_to_repr": (C.c_int, [_P, _P, _SZ, _P]),
    "lh_fr_from_repr": (C.c_int, [_P, _P, _SZ, _P]),
    "lh_fr_add": (C.c_int, [_P, _P, _P, _SZ, _P]),
    "lh_fr_sub": (C.c_int, [_P, _P, _P, _SZ, _P]),
    "lh_fr_mul": (C.c_int, [_P, _P, _P, _SZ, _P]),
    "lh_fr_mul_chain": (C.c_int, [_P, _P, _P, _SZ, C.c_int, _P]),
    "lh_fr_batch_invert": (C.c_int, [_P, _P, _SZ, _P]),
    "lh_fix_var": (C.c_int, [_P, _P, _SZ, C.POINTER(lh_fr), _P]),
    "lh_eq_xy": (C.c_int, [_P, C.POINTER(lh_fr), _SZ, _P]),
    "lh_evaluate": (C.c_int, [_P, C.POINTER(_P), _SZ, _SZ, C.POINTER(lh_fr), C.POINTER(lh_fr)]),
    "lh_lincomb": (C.c_int, [_P, C.POINTER(_P), C.POINTER(lh_fr), _SZ, _SZ, _P]),
    "lh_sumcheck_prove": (C.c_int, [_P, C.c_int, _SZ, C.POINTER(lh_sop), C.POINTER(_P), _SZ,
                                    C.POINTER(lh_fr), _SZ, C.POINTER(lh_fr), C.POINTER(lh_transcript),
                                    C.POINTER(lh_fr), C.POINTER(lh_fr)]),
    "lh_sumcheck_prove_expr": (C.c_int, [_P, _SZ, C.POINTER(lh_expr), C.POINTER(_P), _SZ, C.POINTER(lh_fr), _SZ,
                                         C.POINTER(lh_fr), _SZ, C.POINTER(lh_fr), C.POINTER(lh_transcript),
                                         C.POINTER(lh_fr), C.POINTER(lh_fr)]),
    "lh_gkr_fractional_prove": (C.c_int, [_P, _SZ, _SZ, C.POINTER(C.POINTER(lh_fr)), C.POINTER(C.POINTER(lh_fr)),
                                          C.POINTER(_P), C.POINTER(_P), C.POINTER(lh_transcript),
                                          C.POINTER(lh_fr), C.POINTER(lh_fr), C.POINTER(lh_fr)]),
    "lh_grand_product_prove": (C.c_int, [_P, _SZ, C.POINTER(_P), C.POINTER(_SZ), C.POINTER(lh_transcript),
                                         C.POINTER(lh_fr), C.POINTER(lh_fr), C.POINTER(lh_fr)]),
    "lh_msm": (C.c_int, [_P, _P, _P, _SZ, C.POINTER(lh_g1)]),
    "lh_msm_u32": (C.c_int, [_P, _P, _P, _SZ, C.POINTER(lh_g1)]),
    "lh_mkzg_setup": (C.c_int, [_P, C.POINTER(lh_fr), _SZ, C.POINTER(_P)]),
    "lh_srs_upload": (C.c_int, [_P, _P, _SZ, C.POINTER(_P)]),
    "lh_srs_download": (C.c_int, [_P, _P, _P]),
    "lh_srs_num_vars": (_SZ, [_P]),
    "lh_srs_free": (None, [_P, _P]),
    "lh_mkzg_commit": (C.c_int, [_P, _P, _P, _SZ, C.POINTER(lh_g1)]),
    "lh_mkzg_batch_commit": (C.c_int, [_P, _P, C.POINTER(_P), _SZ, _SZ, C.POINTER(lh_g1)]),
    "lh_mkzg_open": (C.c_int, [_P, _P, _P, _SZ, C.POINTER(lh_fr), C.POINTER(lh_transcript), C.POINTER(lh_fr)]),
    "lh_mkzg_batch_open": (C.c_int, [_P, _P, _SZ, C.POINTER(_P), _SZ, C.POINTER(lh_fr), _SZ,
                                     C.POINTER(lh_evaluation), _SZ, C.POINTER(lh_transcript)]),
    "lh_lasso_last_timing": (C.c_int, [_P, C.POINTER(C.c_double)]),
    "lh_ctx_set_option": (C.c_int, [_P, C.c_char_p, C.c_int64]),
    "lh_ctx_get_option": (C.c_int, [_P, C.c_char_p, C.POINTER(C.c_int64)]),
    "lh_lasso_last_route": (C.c_int, [_P, C.POINTER(C.c_uint32)]),
    "lh_subtable_register": (C.c_int, [C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_uint32)]),
    "lh_subtable_unregister": (C.c_int, [C.c_uint32]),
    "lh_subtable_info": (C.c_int, [C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_char_p]),
    "lh_ctx_set_comm": (C.c_int, [_P, C.POINTER(lh_comm), _SZ]),
    "lh_rccl_unique_id": (C.c_int, [C.c_char_p]),
    "lh_ctx_set_comm_rccl": (C.c_int, [_P, C.c_int, C.c_int, C.c_char_p, _SZ]),
    "lh_ctx_set_comm_loopback": (C.c_int, [_P, C.c_int, C.c_int, _SZ]),
    "lh_ctx_comm_stats": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "lh_ctx_comm_phase_stats": (C.c_int, [_P, C.POINTER(C.c_uint64), C.c_int]),
    "lh_ctx_memory_stats": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "lh_ctx_compute_units": (C.c_int, [_P, C.POINTER(C.c_size_t)]),
    "lh_ctx_host_cpus": (C.c_int, [_P, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]),
    "lh_lasso_prove_sharded": (C.c_int, [_P, _P, C.POINTER(lh_lasso_table), _SZ, C.POINTER(_P),
                                         C.POINTER(lh_transcript)]),
    "lh_shard_extract": (C.c_int, [_P, _P, _SZ, _SZ, _SZ, _SZ, _SZ, _P]),
    "lh_hyperplonk_prove_sharded": (C.c_int, [_P, _P, C.POINTER(lh_hp_param), C.POINTER(C.POINTER(lh_fr)), C.POINTER(_P),
                                              C.POINTER(lh_transcript)]),
    "lh_keccak_transcript_from_proof": (C.c_int, [C.c_char_p, _SZ, C.POINTER(C.POINTER(lh_transcript))]),
    "lh_keccak_transcript_remaining": (C.c_int, [C.POINTER(lh_transcript), C.POINTER(_SZ)]),
    "lh_mkzg_vp_setup": (C.c_int, [C.POINTER(lh_fr), _SZ, C.POINTER(_P)]),
    "lh_mkzg_vp_new": (C.c_int, [C.POINTER(lh_g1), C.POINTER(lh_g2), C.POINTER(lh_g2), _SZ, C.POINTER(_P)]),
    "lh_mkzg_vp_export": (C.c_int, [_P, C.POINTER(lh_g1), C.POINTER(lh_g2), C.POINTER(lh_g2)]),
    "lh_mkzg_vp_num_vars": (_SZ, [_P]),
    "lh_mkzg_vp_free": (None, [_P]),
    "lh_pairing_check": (C.c_int, [C.POINTER(lh_g1), C.POINTER(lh_g2), _SZ, C.POINTER(C.c_int)]),
    "lh_mkzg_verify": (C.c_int, [_P, C.POINTER(lh_g1), C.POINTER(lh_fr), _SZ, C.POINTER(lh_fr),
                                 C.POINTER(lh_transcript)]),
    "lh_mkzg_batch_verify": (C.c_int, [_P, _SZ, C.POINTER(lh_g1), _SZ, C.POINTER(lh_fr), _SZ,
                                       C.POINTER(lh_evaluation), _SZ, C.POINTER(lh_transcript)]),
    "lh_sumcheck_verify": (C.c_int, [C.c_int, _SZ, _SZ, C.POINTER(lh_fr), C.POINTER(lh_transcript),
                                     C.POINTER(lh_fr), C.POINTER(lh_fr)]),
    "lh_ukzg_setup": (C.c_int, [_P, C.POINTER(lh_fr), _SZ, C.POINTER(_P)]),
    "lh_usrs_upload": (C.c_int, [_P, C.c_char_p, _SZ, C.POINTER(_P)]),
    "lh_usrs_download": (C.c_int, [_P, _P, C.c_char_p]),
    "lh_usrs_size": (_SZ, [_P]),
    "lh_usrs_free": (None, [_P, _P]),
    "lh_zeromorph_batch_commit": (C.c_int, [_P, _P, _SZ, C.POINTER(_P), _SZ, _SZ, C.POINTER(lh_g1)]),
    "lh_zeromorph_open": (C.c_int, [_P, _P, _SZ, _P, _SZ, C.POINTER(lh_fr), C.POINTER(lh_transcript)]),
    "lh_zeromorph_batch_open": (C.c_int, [_P, _P, _SZ, _SZ, C.POINTER(_P), _SZ, C.POINTER(lh_fr), _SZ,
                                          C.POINTER(lh_evaluation), _SZ, C.POINTER(lh_transcript)]),
    "lh_zeromorph_vp_setup": (C.c_int, [C.POINTER(lh_fr), _SZ, _SZ, C.POINTER(_P)]),
    "lh_zeromorph_vp_new": (C.c_int, [C.POINTER(lh_g1), C.POINTER(lh_g2), C.POINTER(lh_g2), C.POINTER(lh_g2),
                                      C.POINTER(_P)]),
    "lh_zeromorph_vp_export": (C.c_int, [_P, C.POINTER(lh_g1), C.POINTER(lh_g2), C.POINTER(lh_g2), C.POINTER(lh_g2)]),
    "lh_zeromorph_vp_free": (None, [_P]),
    "lh_zeromorph_verify": (C.c_int, [_P, C.POINTER(lh_g1), C.POINTER(lh_fr), _SZ, C.POINTER(lh_fr),
                                      C.POINTER(lh_transcript)]),
    "lh_zeromorph_batch_verify": (C.c_int, [_P, _SZ, C.POINTER(lh_g1), _SZ, C.POINTER(lh_fr), _SZ,
                                            C.POINTER(lh_evaluation), _SZ, C.POINTER(lh_transcript)]),
    "lh_ukzg_batch_commit": (C.c_int, [_P, _P, _SZ, C.POINTER(_P), C.POINTER(_SZ), _SZ, C.POINTER(lh_g1)]),
    "lh_ukzg_open": (C.c_int, [_P, _P, _SZ, _P, _SZ, C.POINTER(lh_fr), C.POINTER(lh_transcript)]),
    "lh_ukzg_batch_open": (C.c_int, [_P, _P, _SZ, C.POINTER(_P), C.POINTER(_SZ), _SZ, C.POINTER(lh_fr), _SZ,
                                     C.POINTER(lh_evaluation), _SZ, C.POINTER(lh_transcript)]),
    "lh_ukzg_vp_setup": (C.c_int, [C.POINTER(lh_fr), C.POINTER(_P)]),
    "lh_ukzg_vp_new": (C.c_int, [C.POINTER(lh_g1), C.POINTER(lh_g2), C.POINTER(lh_g2), C.POINTER(_P)]),
    "lh_ukzg_vp_export": (C.c_int, [_P, C.POINTER(lh_g1), C.POINTER(lh_g2), C.POINTER(lh_g2)]),
    "lh_ukzg_vp_free": (None, [_P]),
    "lh_ukzg_verify": (C.c_int, [_P, C.POINTER(lh_g1), C.POINTER(lh_fr), C.POINTER(lh_fr), C.POINTER(lh_transcript)]),
    "lh_ukzg_batch_verify": (C.c_int, [_P, C.POINTER(lh_g1), _SZ, C.POINTER(lh_fr), _SZ, C.POINTER(lh_evaluation), _SZ,
                                       C.POINTER(lh_transcript)]),
    "lh_gemini_batch_commit": (C.c_int, [_P, _P, _SZ, C.POINTER(_P), _SZ, _SZ, C.POINTER(lh_g1)]),
    "lh_gemini_open": (C.c_int, [_P, _P, _SZ, _P, _SZ, C.POINTER(lh_fr), C.POINTER(lh_transcript)]),
    "lh_gemini_batch_open": (C.c_int, [_P, _P, _SZ, _SZ, C.POINTER(_P), _SZ, C.POINTER(lh_fr), _SZ,
                                       C.POINTER(lh_evaluation), _SZ, C.POINTER(lh_transcript)]),
    "lh_gemini_folds": (C.c_int, [_P, _P, _SZ, C.POINTER(lh_fr), _P]),
    "lh_gemini_verify": (C.c_int, [_P, C.POINTER(lh_g1), C.POINTER(lh_fr), _SZ, C.POINTER(lh_fr),
                                   C.POINTER(lh_transcript)]),
    "lh_gemini_batch_verify": (C.c_int, [_P, _SZ, C.POINTER(lh_g1), _SZ, C.POINTER(lh_fr), _SZ,
                                         C.POINTER(lh_evaluation), _SZ, C.POINTER(lh_transcript)]),
    "lh_ipa_setup": (C.c_int, [_P, _SZ, C.POINTER(_P)]),
    "lh_ipa_param_free": (None, [_P, _P]),
    "lh_ipa_param_size": (_SZ, [_P]),
    "lh_ipa_param_download": (C.c_int, [_P, _P, C.c_char_p, C.POINTER(lh_g1)]),
    "lh_ipa_batch_commit": (C.c_int, [_P, _P, _SZ, C.POINTER(_P), _SZ, _SZ, C.POINTER(lh_g1)]),
    "lh_ipa_open": (C.c_int, [_P, _P, _SZ, _P, _SZ, C.POINTER(lh_fr), C.POINTER(lh_transcript)]),
    "lh_ipa_batch_open": (C.c_int, [_P, _P, _SZ, _SZ, C.POINTER(_P), _SZ, C.POINTER(lh_fr), _SZ,
                                    C.POINTER(lh_evaluation), _SZ, C.POINTER(lh_transcript)]),
    "lh_ipa_verify": (C.c_int, [_P, _SZ, C.POINTER(lh_g1), C.POINTER(lh_fr), _SZ, C.POINTER(lh_fr),
                                C.POINTER(lh_transcript)]),
    "lh_ipa_batch_verify": (C.c_int, [_P, _SZ, _SZ, C.POINTER(lh_g1), _SZ, C.POINTER(lh_fr), _SZ,
                                      C.POINTER(lh_evaluation), _SZ, C.POINTER(lh_transcript)]),
    "lh_g1_axpy": (C.c_int, [_P, _P, _P, _SZ, C.POINTER(lh_fr), _P]),
    "lh_g1_rows_msm": (C.c_int, [_P, _P, C.c_int, C.c_uint32, _SZ, _SZ, _P, C.POINTER(lh_g1)]),
    "lh_hyrax_setup": (C.c_int, [_P, _SZ, _SZ, C.POINTER(_P)]),
    "lh_hyrax_dims": (C.c_int, [_SZ, _SZ, C.POINTER(_SZ), C.POINTER(_SZ), C.POINTER(_SZ)]),
    "lh_hyrax_trim": (C.c_int, [_P, _SZ, _SZ, C.POINTER(_SZ), C.POINTER(_SZ)]),
    "lh_hyrax_batch_commit": (C.c_int, [_P, _P, _SZ, _SZ, C.POINTER(_P), _SZ, _SZ, C.POINTER(lh_g1)]),
    "lh_hyrax_open": (C.c_int, [_P, _P, _SZ, _SZ, _P, _SZ, C.POINTER(lh_fr), C.POINTER(lh_transcript)]),
    "lh_hyrax_batch_open": (C.c_int, [_P, _P, _SZ, _SZ, _SZ, C.POINTER(_P), _SZ, C.POINTER(lh_fr), _SZ,
                                      C.POINTER(lh_evaluation), _SZ, C.POINTER(lh_transcript)]),
    "lh_hyrax_verify": (C.c_int, [_P, _SZ, _SZ, C.POINTER(lh_g1), C.POINTER(lh_fr), _SZ, C.POINTER(lh_fr),
                                  C.POINTER(lh_transcript)]),
    "lh_hyrax_batch_verify": (C.c_int, [_P, _SZ, _SZ, _SZ, C.POINTER(lh_g1), _SZ, C.POINTER(lh_fr), _SZ,
                                        C.POINTER(lh_evaluation), _SZ, C.POINTER(lh_transcript)]),
    "lh_debug_jit_source": (C.c_int, [C.POINTER(C.c_uint32), _SZ, C.c_uint32, C.c_uint32, C.c_int, C.c_char_p, _SZ,
                                      C.POINTER(_SZ)]),
    "lh_debug_sort_pairs": (C.c_int, [_P, C.c_int, C.POINTER(lh_debug_sort_slab), _SZ]),
    "lh_debug_lasso_counters": (C.c_int, [_P, C.POINTER(_P), _SZ, _SZ, _SZ, C.POINTER(_P), C.POINTER(_P), C.POINTER(_P),
                                          C.POINTER(_P)]),
    "lh_debug_sort_plan": (C.c_int, [_SZ, C.c_uint, C.c_int, C.POINTER(C.c_uint), C.POINTER(C.c_uint), C.POINTER(_SZ)]),
    "lh_debug_msm_plan": (C.c_int, [_SZ, C.POINTER(_SZ), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_int, C.c_int,
                                    C.POINTER(C.c_uint64), C.POINTER(_SZ)]),
    "lh_debug_live_resources": (C.c_int, [C.POINTER(C.c_uint64)]),
    "lh_debug_fail_acquire_after": (C.c_int, [C.c_int64]),
    "lh_debug_u32_columns": (C.c_int, [_P, C.c_int, C.POINTER(lh_debug_u32_args)]),
    "lh_debug_lasso_subtable_read": (C.c_int, [_P, C.c_uint32, C.c_uint32, _P, _SZ, _P]),
    "lh_keccak_transcript_hash_io": (C.c_int, [C.POINTER(lh_transcript), C.POINTER(lh_hash_transcript)]),
    "lh_brakedown_setup": (C.c_int, [_P, _SZ, C.c_int, C.c_char_p, C.POINTER(_P)]),
    "lh_brakedown_derive": (C.c_int, [_SZ, C.c_int, C.POINTER(_P)]),
    "lh_ligero_setup": (C.c_int, [_P, _SZ, C.c_int, _SZ, C.POINTER(_P)]),
    "lh_ligero_derive": (C.c_int, [_SZ, C.c_int, _SZ, C.POINTER(_P)]),
    "lh_brakedown_param_info": (C.c_int, [_P, C.POINTER(_SZ), C.POINTER(_SZ), C.POINTER(_SZ), C.POINTER(_SZ),
                                          C.POINTER(_SZ)]),
    "lh_brakedown_trim": (C.c_int, [_P, _SZ]),
    "lh_brakedown_param_free": (None, [_P]),
    "lh_brakedown_encode": (C.c_int, [_P, C.POINTER(lh_fr), C.POINTER(lh_fr)]),
    "lh_brakedown_commit": (C.c_int, [_P, _P, _P, _SZ, C.POINTER(_P)]),
    "lh_brakedown_batch_commit": (C.c_int, [_P, _P, C.POINTER(_P), _SZ, _SZ, C.POINTER(_P)]),
    "lh_brakedown_commit_columns": (C.c_int, [_P, _P, C.POINTER(_P), C.POINTER(C.c_int), C.POINTER(_SZ), _SZ, C.POINTER(_P)]),
    "lh_brakedown_comm_root": (C.c_int, [_P, C.c_char_p]),
    "lh_brakedown_comm_rows": (C.c_int, [_P, _P, _P]),
    "lh_brakedown_comm_rows_device": (C.c_int, [_P, C.POINTER(_P)]),
    "lh_brakedown_comm_tree": (C.c_int, [_P, _P, C.c_char_p]),
    "lh_brakedown_comm_stage": (C.c_int, [_P, _P, _P, _P]),
    "lh_brakedown_comm_free": (None, [_P]),
    "lh_hyperplonk_prove_brakedown": (C.c_int, [_P, _P, C.POINTER(lh_hp_param), C.POINTER(_P), C.POINTER(_P),
                                                C.POINTER(C.POINTER(lh_fr)), C.POINTER(_P), C.POINTER(lh_transcript),
                                                C.POINTER(lh_hash_transcript)]),
    "lh_hyperplonk_prove_phases_brakedown": (C.c_int, [_P, _P, C.POINTER(lh_hp_param), C.POINTER(_P), C.POINTER(_P), _SZ,
                                                       C.POINTER(_SZ), C.POINTER(_SZ), C.POINTER(C.POINTER(lh_fr)),
                                                       C.POINTER(lh_hp_circuit), C.POINTER(lh_transcript),
                                                       C.POINTER(lh_hash_transcript)]),
    "lh_hyperplonk_verify_brakedown": (C.c_int, [_P, C.POINTER(lh_hp_vparam), C.c_char_p, C.c_char_p,
                                                 C.POINTER(C.POINTER(lh_fr)), C.POINTER(lh_transcript),
                                                 C.POINTER(lh_hash_transcript)]),
    "lh_hyperplonk_verify_phases_brakedown": (C.c_int, [_P, C.POINTER(lh_hp_vparam), C.c_char_p, C.c_char_p, _SZ,
                                                        C.POINTER(_SZ), C.POINTER(_SZ), C.POINTER(C.POINTER(lh_fr)),
                                                        C.POINTER(lh_transcript), C.POINTER(lh_hash_transcript)]),
    "lh_brakedown_open": (C.c_int, [_P, _P, _P, _SZ, _P, C.POINTER(lh_fr), C.POINTER(lh_transcript),
                                    C.POINTER(lh_hash_transcript)]),
    "lh_brakedown_batch_open": (C.c_int, [_P, _P, _SZ, C.POINTER(_P), C.POINTER(_P), _SZ, C.POINTER(lh_fr), _SZ,
                                          C.POINTER(lh_evaluation), _SZ, C.POINTER(lh_transcript),
                                          C.POINTER(lh_hash_transcript)]),
    "lh_brakedown_read_commitments": (C.c_int, [_P, _SZ, C.POINTER(lh_hash_transcript), C.c_char_p]),
    "lh_brakedown_verify": (C.c_int, [_P, C.c_char_p, C.POINTER(lh_fr), _SZ, C.POINTER(lh_fr), C.POINTER(lh_transcript),
                                      C.POINTER(lh_hash_transcript)]),
    "lh_brakedown_batch_verify": (C.c_int, [_P, _SZ, C.c_char_p, _SZ, C.POINTER(lh_fr), _SZ, C.POINTER(lh_evaluation),
                                            _SZ, C.POINTER(lh_transcript), C.POINTER(lh_hash_transcript)]),
    "lh_profile_enable": (C.c_int, [_P, C.c_int]),
    "lh_profile_read": (C.c_int, [_P, C.POINTER(lh_prof_rec), _SZ, C.POINTER(_SZ)]),
}

# Lasso and HyperPlonk exist once per point commitment scheme: lh_<kind><suffix>([ctx,] <the scheme's head>, <the kind's tail>)
_PCS_HEADS = {  # suffix -> (prover param, verifier param)
    "": ([_P], [_P]),
    "_zeromorph": ([_P, _SZ], [_P]),
    "_gemini": ([_P, _SZ], [_P]),
    "_ipa": ([_P, _SZ], [_P, _SZ]),
    "_hyrax": ([_P, _SZ, _SZ], [_P, _SZ, _SZ]),
}
_T, _INSTANCES, _PHASES = C.POINTER(lh_transcript), C.POINTER(C.POINTER(lh_fr)), [_SZ, C.POINTER(_SZ), C.POINTER(_SZ)]
_HT = C.POINTER(lh_hash_transcript)  # Brakedown's entries end in it: roots and Merkle paths are no field elements
_PROVE_TAILS = {
    "lh_lasso_prove": [C.POINTER(lh_lasso_table), _SZ, C.POINTER(_P), _T],
    "lh_hyperplonk_prove": [C.POINTER(lh_hp_param), _INSTANCES, C.POINTER(_P), _T],
    "lh_hyperplonk_prove_phases": [C.POINTER(lh_hp_param)] + _PHASES + [_INSTANCES, C.POINTER(lh_hp_circuit), _T],
}
_VERIFY_TAILS = {
    "lh_lasso_verify": [C.POINTER(lh_lasso_table), _SZ, _T],
    "lh_hyperplonk_verify": [C.POINTER(lh_hp_vparam), _INSTANCES, _T],
    "lh_hyperplonk_verify_phases": [C.POINTER(lh_hp_vparam)] + _PHASES + [_INSTANCES, _T],
}
for _suffix, (_prover, _verifier) in _PCS_HEADS.items():
    for _kind, _tail in _PROVE_TAILS.items():
        SIGNATURES[_kind + _suffix] = (C.c_int, [_P] + _prover + _tail)
    for _kind, _tail in _VERIFY_TAILS.items():
        SIGNATURES[_kind + _suffix] = (C.c_int, _verifier + _tail)

# Lasso over Brakedown: the same tails behind the param, the hash transcript behind them
SIGNATURES["lh_lasso_prove_brakedown"] = (C.c_int, [_P, _P] + _PROVE_TAILS["lh_lasso_prove"] + [_HT])
SIGNATURES["lh_lasso_verify_brakedown"] = (C.c_int, [_P] + _VERIFY_TAILS["lh_lasso_verify"] + [_HT])

# several tables in one proof (multilinear KZG): lists of table pointers, and per table a list of chunk column pointers
LH_LASSO_BATCH_MAX_TABLES = 8
SIGNATURES["lh_lasso_prove_batch"] = (C.c_int, [_P, _P, C.POINTER(C.POINTER(lh_lasso_table)), _SZ, _SZ,
                                                C.POINTER(C.POINTER(_P)), _T])
SIGNATURES["lh_lasso_verify_batch"] = (C.c_int, [_P, C.POINTER(C.POINTER(lh_lasso_table)), _SZ, _SZ, _T])
SIGNATURES["lh_logup_gkr_prove"] = (C.c_int, [_P, _P, C.POINTER(lh_logup_lookup), _SZ, _SZ, _SZ, _T])
SIGNATURES["lh_logup_gkr_prove_columns"] = (C.c_int, [_P, _P, C.POINTER(lh_logup_columns), _SZ, _SZ, _SZ, _T])
SIGNATURES["lh_logup_gkr_verify"] = (C.c_int, [_P, C.POINTER(lh_logup_lookup), _SZ, _SZ, _SZ, _T])
SIGNATURES["lh_memcheck_prove"] = (C.c_int, [_P, _P, C.POINTER(lh_memcheck_trace), _SZ, _SZ, C.POINTER(C.c_uint32), _T])
SIGNATURES["lh_memcheck_verify"] = (C.c_int, [_P, _SZ, _SZ, C.POINTER(C.c_uint32), _T])
SIGNATURES["lh_debug_memcheck_witness"] = (C.c_int, [_P, C.POINTER(lh_memcheck_trace), _SZ, _SZ, C.POINTER(C.c_uint32), _P, _P, _P,
                                                     _P, C.POINTER(C.c_int)])
# (d_image, d_rv, d_wv, d_final: device pointers)
SIGNATURES["lh_memcheck_replay"] = (C.c_int, [_P, C.POINTER(lh_memcheck_ops), _SZ, _SZ, _P, _P, _P, _P])
SIGNATURES["lh_memcheck_prove_segment"] = (C.c_int, [_P, _P, C.POINTER(lh_memcheck_trace), _SZ, _SZ, _P, _P, _T])
SIGNATURES["lh_memcheck_verify_segment"] = (C.c_int, [_P, _SZ, _SZ, _T, C.POINTER(lh_g1), C.POINTER(lh_g1)])
# Spark: the handle is an opaque pointer; lh_spark_free returns nothing
SIGNATURES["lh_spark_commit"] = (C.c_int, [_P, _P, _SZ, _SZ, _SZ, _P, _P, C.POINTER(_P)])
SIGNATURES["lh_spark_commitment"] = (C.c_int, [_P, _P, C.POINTER(_SZ)])
SIGNATURES["lh_spark_open"] = (C.c_int, [_P, _P, _P, C.POINTER(lh_fr), C.POINTER(lh_fr), _T])
SIGNATURES["lh_spark_free"] = (None, [_P, _P])
SIGNATURES["lh_spark_verify"] = (C.c_int, [_P, _SZ, _SZ, _SZ, _P, _SZ, C.POINTER(lh_fr), C.POINTER(lh_fr), _T])
SIGNATURES["lh_debug_spark_e"] = (C.c_int, [_P, _SZ, _SZ, _SZ, _P, _P, C.POINTER(lh_fr), _P, C.POINTER(lh_fr)])
# Spartan: the key is an opaque pointer; lh_r1cs_free returns nothing
SIGNATURES["lh_r1cs_commit"] = (C.c_int, [_P, _P, _SZ, _SZ, C.POINTER(lh_r1cs_matrix), C.POINTER(_P)])
SIGNATURES["lh_r1cs_commitment"] = (C.c_int, [_P, _P, C.POINTER(_SZ)])
SIGNATURES["lh_spartan_prove"] = (C.c_int, [_P, _P, _P, C.POINTER(lh_fr), C.POINTER(lh_fr), _SZ, _T])
SIGNATURES["lh_r1cs_free"] = (None, [_P, _P])
SIGNATURES["lh_spartan_verify"] = (C.c_int, [_P, _SZ, _SZ, _P, _SZ, C.POINTER(lh_fr), _SZ, _T])
SIGNATURES["lh_debug_spartan_spmv"] = (C.c_int, [_P, _P, C.c_int, C.POINTER(lh_fr), C.POINTER(C.POINTER(lh_fr))])
# Nova folding: instance blobs in and out as bytes (out: the buffer and its room in / length out)
_FR = C.POINTER(lh_fr)
SIGNATURES["lh_nova_instance"] = (C.c_int, [_P, _P, _P, _FR, _FR, _SZ, _P, C.POINTER(_SZ)])
SIGNATURES["lh_nova_fold"] = (C.c_int, [_P, _P, _P, _P, _SZ, _P, _SZ, _FR, _FR, _FR, _FR, _FR, _FR, _P, C.POINTER(_SZ), _T])
SIGNATURES["lh_spartan_prove_relaxed"] = (C.c_int, [_P, _P, _P, _P, _SZ, _FR, _FR, _T])
SIGNATURES["lh_nova_fold_verify"] = (C.c_int, [_SZ, _SZ, _P, _SZ, _P, _SZ, _P, _SZ, _P, C.POINTER(_SZ), _T])
SIGNATURES["lh_spartan_verify_relaxed"] = (C.c_int, [_P, _SZ, _SZ, _P, _SZ, _P, _SZ, _SZ, _T])
SIGNATURES["lh_debug_nova_spmv2"] = (C.c_int, [_P, _P, C.c_int, _FR, _FR, C.POINTER(_FR), C.POINTER(_FR)])
SIGNATURES["lh_debug_nova_cross_term"] = (C.c_int, [_P, _SZ, C.POINTER(_FR), C.POINTER(_FR), _FR, _FR, _FR, _FR, _FR, C.POINTER(_SZ)])
SIGNATURES["lh_debug_nova_fold"] = (C.c_int, [_P, _SZ, _FR, _FR, _FR, _FR, _FR, _FR, _FR, _FR])
# batched Spartan, the verifier: the public inputs instance by instance
SIGNATURES["lh_spartan_verify_batch"] = (C.c_int, [_P, _SZ, _SZ, _P, _SZ, _FR, _SZ, _SZ, _T])
SIGNATURES["lh_gkr_fractional_verify"] = (C.c_int, [_SZ, _SZ, C.POINTER(C.POINTER(lh_fr)), C.POINTER(C.POINTER(lh_fr)), _T,
                                                    C.POINTER(lh_fr), C.POINTER(lh_fr), C.POINTER(lh_fr), C.POINTER(lh_fr),
                                                    C.POINTER(lh_fr)])

_lib = None


def load():
    """dlopen the in-tree library and attach the signatures; raises if it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(no CPU fallback exists)" % LIB_PATH)
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib
