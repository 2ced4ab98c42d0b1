// Brakedown PCS (reference pcs/multilinear/brakedown.rs, util/code/brakedown.rs): parameters, the seeded matrix
// sampler, the host encoder, and the device-resident commitment.  Kernels in kernels_brakedown.hip; the prover half in
// brakedown.cpp, the verifier in verifier.cpp.  DESIGN.md §12.
#pragma once
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
};

struct BdParam {
  size_t num_vars = 0, n_0 = 0, row_len = 0, num_rows = 0, codeword_len = 0, num_column_opening = 0,
         num_proximity_testing = 0, depth = 0;
  int spec = 0;
  std::vector<BdMatrix> a, b;
  int device = -1;  // >= 0: the matrices are on this device too
  ~BdParam();
};

// MultilinearBrakedownCommitment: the encoded rows and the Merkle tree stay on the device
struct BdComm {
  size_t num_rows = 0, codeword_len = 0, depth = 0;
  int device = -1;
  Fr* d_rows = nullptr;         // num_rows x codeword_len, row-major
  uint64_t* d_hashes = nullptr; // (2 << depth) - 1 digests of 4 words: leaves, then each level up, the root last
  uint8_t root[32];
  std::vector<uint64_t> host_tree;  // filled by the first open: the paths are read on the host
  ~BdComm();
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
BdParam* brakedown_setup(Ctx* c, size_t num_vars, int spec, const uint8_t seed[32]);
void brakedown_trim(const BdParam& p, size_t poly_size);
// LinearCodes::encode: `cw` holds the message in its first row_len entries and gets the codeword
void brakedown_encode_host(const BdParam& p, HFr* cw);
BdComm* brakedown_commit(Ctx& c, const BdParam& p, const Fr* d_poly, size_t num_vars);
void brakedown_open(Ctx& c, const BdParam& p, const Fr* d_poly, size_t num_vars, BdComm& comm, const HFr* point,
                    Transcript& tr, HashTranscript& ht);
void brakedown_verify(const BdParam& p, const uint8_t root[32], const HFr* point, size_t num_vars, const HFr& eval,
                      Transcript& tr, HashTranscript& ht);

// kernels_brakedown.hip
void k_bd_gather(Ctx&, Fr* rows, size_t num_rows, size_t cw, size_t in_off, size_t out_off, const BdMatrix& mat);
void k_bd_reed_solomon(Ctx&, Fr* rows, size_t num_rows, size_t cw, size_t in_off, const BdMatrix& a_last, size_t bn);
void k_bd_hash_columns(Ctx&, const Fr* rows, size_t num_rows, size_t cw, size_t width, uint64_t* leaves);
void k_bd_merkle_level(Ctx&, const uint64_t* in, size_t out_n, uint64_t* out);
void k_bd_combine(Ctx&, const Fr* poly, size_t num_rows, size_t row_len, const Fr* coeffs, int num_sets, Fr* out);

}  // namespace lh
