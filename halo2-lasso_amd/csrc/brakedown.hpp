// Brakedown PCS (reference pcs/multilinear/brakedown.rs, util/code/brakedown.rs): parameters, the seeded matrix
// sampler, the host encoder, and the device-resident commitment.  Kernels in kernels_brakedown.hip; the prover half in
// brakedown.cpp, the verifier in verifier.cpp.  DESIGN.md §12.
#pragma once
#include <memory>
#include "host.hpp"

namespace lh {

struct BdDim {
  size_t n, m, d;  // SparseMatrixDimension (code/brakedown.rs:262-266)
};

// SparseMatrix<Fr>: n rows (one per input entry) of d cells (column = output index, coeff), columns ascending
struct BdMatrix {
  BdDim dim;
  std::vector<uint32_t> cols;  // n * d
  std::vector<HFr> coeffs;     // n * d
  // device copy (setup with a ctx), transposed: CSR grouped by output index, inputs ascending within a group
  uint32_t* d_ptr = nullptr;  // m + 1
  uint32_t* d_idx = nullptr;  // nnz input indices
  Fr* d_val = nullptr;        // nnz coefficients
  DevMem mem[3];              // the blocks behind them
};

struct BdParam {
  size_t num_vars = 0, n_0 = 0, row_len = 0, num_rows = 0, codeword_len = 0, num_column_opening = 0,
         num_proximity_testing = 0, depth = 0;
  int spec = 0;
  std::vector<BdMatrix> a, b;
  int device = -1;  // >= 0: the matrices (or the twiddle table) are on this device too
  // The code the rows are encoded with.  BD_CODE_RS (ligero_derive / ligero_setup): a systematic
  // Reed-Solomon code of rate 2^-log_inv_rate over the 2^depth-th roots of unity; no matrices, `spec` is 0 and n_0 unused.
  int code = 0;  // BD_CODE_EXPANDER
  int log_inv_rate = 0;
  std::vector<HFr> tw;  // w_N^t for t < codeword_len (setup; a derived param has none)
  Fr* d_tw = nullptr;   // the same table on the device (setup with a ctx)
  DevMem tw_mem;
};
enum { BD_CODE_EXPANDER = 0, BD_CODE_RS = 1 };
constexpr size_t LIGERO_ROW_VARS_AUTO = (size_t)-1;
constexpr size_t LIGERO_MAX_DEVICE_ROW_VARS = 22;  // the longest row k_bd_rs_encode takes (two passes of 2^11)

// MultilinearBrakedownCommitment: the encoded rows and the Merkle tree stay on the device
struct BdComm {
  size_t num_rows = 0, codeword_len = 0, depth = 0;
  int device = -1;
  Fr* d_rows = nullptr;         // num_rows x codeword_len, row-major
  uint64_t* d_hashes = nullptr; // (2 << depth) - 1 digests of 4 words: leaves, then each level up, the root last
  uint8_t root[32];
  std::vector<uint64_t> host_tree;  // filled by the first open: the paths are read on the host
  DevMem rows_mem, hashes_mem;  // a commitment of its own (brakedown_commit): the blocks behind d_rows and d_hashes
  // a commitment of a batch (brakedown_batch_commit): d_rows / d_hashes point into the batch's one allocation, which the
  // last commitment of the batch frees; or into memory the caller owns (`borrowed`: an arena slab of a proof)
  std::shared_ptr<DevMem> slab;
  bool borrowed = false;
};

// The encoded matrix of ONE commitment on the host, column-major (column c's num_rows entries at c * num_rows), in pinned
// memory: every column of every open of that commitment is then a host read (brakedown_open's `staged`).  Staging another
// commitment replaces it; the buffer grows to the largest matrix staged and is freed with this object.
struct BdStage {
  const BdComm* of = nullptr;
  PinnedMem cols;  // HFr entries
};

// TranscriptWrite / TranscriptRead<Output<Keccak256>, Fr> (util/transcript.rs:240-265): raw 32 bytes, not absorbed
struct HashTranscript {
  lh_hash_transcript* h;
  explicit HashTranscript(lh_hash_transcript* h_) : h(h_) {
    LH_REQUIRE(h && h->write_hash && h->read_hash, LH_ERR_ARG, "hash transcript callback table is incomplete");
  }
  void check(int rc) {
    if (rc != LH_OK) throw Error(rc, get_last_error()[0] ? get_last_error() : "hash transcript callback failed");
  }
  void write_hash(const uint8_t* hash) { check(h->write_hash(h->user, hash)); }
  void read_hash(uint8_t* out) { check(h->read_hash(h->user, out)); }
};

// fills `out` for the built-in Keccak256Transcript; false for any other callback table
bool keccak_transcript_hash_io(lh_transcript* t, lh_hash_transcript* out);

// parameters only (no matrices): throws LH_ERR_ARG where the reference panics
void brakedown_derive(BdParam& p, size_t num_vars, int spec);
BdParam brakedown_setup(Ctx* c, size_t num_vars, int spec, const uint8_t seed[32]);
// The Ligero PCS: the same scheme over the Reed-Solomon code (tests/ligero_ref.py).  `row_vars` LIGERO_ROW_VARS_AUTO: the
// row length of the smallest proof.  Throws LH_ERR_ARG for log_inv_rate outside 1..3, num_vars outside 1..26,
// row_vars > num_vars and row_vars + log_inv_rate > 28.  Setup needs no seed: the table of roots is all there is.
void ligero_derive(BdParam& p, size_t num_vars, int log_inv_rate, size_t row_vars);
BdParam ligero_setup(Ctx* c, size_t num_vars, int log_inv_rate, size_t row_vars);
void brakedown_trim(const BdParam& p, size_t poly_size);
// LinearCodes::encode: `cw` holds the message in its first row_len entries and gets the codeword
void brakedown_encode_host(const BdParam& p, HFr* cw);
std::unique_ptr<BdComm> brakedown_commit(Ctx& c, const BdParam& p, const Fr* d_poly, size_t num_vars);
// P commits in the launches of one (kernels_brakedown.hip): rows, trees and roots bit-identical to P brakedown_commit
// calls, the roots back in one copy.  `slab` null: one allocation for the batch, shared by the commitments; otherwise the
// caller's memory of brakedown_batch_bytes (256-byte aligned), which outlives them.
size_t brakedown_batch_bytes(const BdParam& p, size_t num_polys);
std::vector<std::unique_ptr<BdComm>> brakedown_batch_commit(Ctx& c, const BdParam& p, const Fr* const* d_polys,
                                                            size_t num_polys, size_t num_vars, void* slab = nullptr);
// A column of a column commit (brakedown_commit_columns): `len` <= 2^num_vars entries on the device, Fr (Montgomery) or u32,
// committed as the table zero-padded to num_vars variables.  The kernels read this table from device memory.
struct BdColumn {
  const void* data;  // may be null when len == 0
  uint64_t len;
  uint32_t u32;  // 1: 4-byte integers, 0: field elements
  uint32_t reserved;
};
// The commits of brakedown_batch_commit without a field-element table per column: the load converts u32 entries to
// Montgomery form and zero-fills from `len` on, and under option brakedown_u32_gather the first encoder stage of the u32
// columns reads the 4-byte entries themselves (kernels_brakedown.hip bd_gather_u32).  Rows, trees and roots are
// bit-identical to brakedown_batch_commit of the zero-padded tables.  `slab` as there, of brakedown_columns_bytes.
size_t brakedown_columns_bytes(const BdParam& p, size_t num_cols);
std::vector<std::unique_ptr<BdComm>> brakedown_commit_columns(Ctx& c, const BdParam& p, const BdColumn* cols,
                                                              size_t num_cols, void* slab = nullptr);
// `d_poly` null: the polynomial is read from the commitment's own rows (the first row_len entries of each row).
// `staged` (optional): the commitment's matrix on the host (brakedown_stage): the column openings read it instead of
// fetching every column from the device; the bytes written are the same
void brakedown_open(Ctx& c, const BdParam& p, const Fr* d_poly, size_t num_vars, BdComm& comm, const HFr* point,
                    Transcript& tr, HashTranscript& ht, const BdStage* staged = nullptr);
// bd_stage_columns, then one device-to-host copy (num_rows == 1: the row itself, no launch); a no-op when `comm` is staged
void brakedown_stage(Ctx& c, const BdParam& p, const BdComm& comm, BdStage& st);
void brakedown_verify(const BdParam& p, const uint8_t root[32], const HFr* point, size_t num_vars, const HFr& eval,
                      Transcript& tr, HashTranscript& ht);

// HyperPlonk over Brakedown (DESIGN.md §12 "Provers").  The Pcs of the prover: commit_and_write commits a phase's polys as
// one batch into an arena slab of the proof's scope and writes the raw roots through `ht` (no Fiat-Shamir state changes);
// batch_open is one open per evaluation in order (brakedown.rs:278-300), the commitment of a poly found by its device
// pointer - the ones made here, or `given` (the preprocess and permutation polys, committed once by the caller) - and its
// columns read from the staged matrix.  What the proof committed, and the pinned staging, go with the returned object.
// commit_columns_and_write (Lasso) commits a proof's columns as ONE batch into one arena slab (brakedown_commit_columns;
// columns that share a data pointer once), writes a root per column and keeps the commitments under the columns' device
// pointers: batch_open looks a poly up by its SmallPoly pointer first and then combines from the commitment's own rows.
struct BdGiven {
  const Fr* d_poly;
  BdComm* comm;
};
Pcs brakedown_pcs(Ctx& c, const BdParam& p, HashTranscript& ht, const std::vector<BdGiven>& given);
// refuses (LH_ERR_ARG) Lasso lookups, a sharded ctx and a circuit of another size than the param's
void brakedown_hyperplonk_prove_phases(Ctx& c, const BdParam& p, const lh_hp_param& pp, BdComm* const* preprocess_comms,
                                       BdComm* const* permutation_comms, const HpPhases& ph, const HFr* const* instances,
                                       Transcript& tr, HashTranscript& ht);
// Lasso over Brakedown (DESIGN.md §12 "Provers"): oracle/pyref/lasso.py prove / verify with the roots written by write_hash.
// Refuses (LH_ERR_ARG) a param whose num_vars is not max(num_vars, chunk_bits) and a ctx inside a sharded prove.
void brakedown_lasso_prove(Ctx& c, const BdParam& p, const lh_lasso_table& table, size_t num_vars,
                           const uint32_t* const* d_dims, Transcript& tr, HashTranscript& ht);
void brakedown_lasso_verify(const BdParam& p, const lh_lasso_table& table, size_t num_vars, Transcript& tr,
                            HashTranscript& ht);  // verifier.cpp
// verifier.cpp: the roots of the witness, m, h and z polys read with read_hash, the preprocess and permutation roots from
// the caller (vp's two lh_g1 arrays are ignored), brakedown_verify once per evaluation
void brakedown_hyperplonk_verify_phases(const BdParam& p, const lh_hp_vparam& vp, const uint8_t* preprocess_roots,
                                        const uint8_t* permutation_roots, const std::vector<size_t>& num_witness_polys,
                                        const std::vector<size_t>& num_challenges, const HFr* const* instances,
                                        Transcript& tr, HashTranscript& ht);

// kernels_brakedown.hip
void k_bd_gather(Ctx&, Fr* rows, size_t num_rows, size_t cw, size_t in_off, size_t out_off, const BdMatrix& mat);
void k_bd_reed_solomon(Ctx&, Fr* rows, size_t num_rows, size_t cw, size_t in_off, const BdMatrix& a_last, size_t bn);
void k_bd_hash_columns(Ctx&, const Fr* rows, size_t num_rows, size_t cw, size_t width, uint64_t* leaves);
void k_bd_merkle_level(Ctx&, const uint64_t* in, size_t out_n, uint64_t* out);
void k_bd_load_rows(Ctx&, const Fr* const* d_polys, size_t num_polys, size_t num_rows, size_t row_len, size_t cw, Fr* rows);
void k_bd_hash_columns_batch(Ctx&, const Fr* rows, size_t num_polys, size_t num_rows, size_t cw, size_t width,
                             uint64_t* trees, size_t tree_stride);
void k_bd_merkle_level_batch(Ctx&, uint64_t* trees, size_t num_polys, size_t tree_stride, size_t in_off, size_t out_n,
                             size_t out_off);
void k_bd_gather_roots(Ctx&, const uint64_t* trees, size_t num_polys, size_t tree_stride, size_t root_off, uint64_t* out);
void k_bd_stage_columns(Ctx&, const Fr* rows, size_t num_rows, size_t cw, Fr* out);
// `stride`: entries between the rows of `poly` (row_len for a table, codeword_len for a commitment's rows)
void k_bd_combine(Ctx&, const Fr* poly, size_t num_rows, size_t row_len, size_t stride, const Fr* coeffs, int num_sets,
                  Fr* out);
void k_bd_load_columns(Ctx&, const BdColumn* d_cols, size_t num_cols, size_t num_rows, size_t row_len, size_t cw, Fr* rows);
// the first forward stage (a[0]: inputs at 0, outputs at row_len) of the u32 columns of the table; Fr columns are left alone
void k_bd_gather_u32(Ctx&, const BdColumn* d_cols, size_t num_cols, Fr* rows, size_t num_rows, size_t row_len, size_t cw,
                     const BdMatrix& mat);

// kernels_ntt.hip: the Reed-Solomon encoder, every row of a slab in place (the message in a row's first 2^row_vars
// entries, coset i of the codeword at i << row_vars).  `twiddles`: w_N^t, t < 2^(row_vars + log_inv_rate), on the device.
void k_bd_rs_encode(Ctx&, Fr* rows, size_t num_rows_total, size_t cw, size_t row_vars, int log_inv_rate,
                    const Fr* twiddles);

}  // namespace lh
