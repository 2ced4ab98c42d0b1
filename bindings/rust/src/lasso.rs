//! The Lasso lookup argument (no counterpart in the reference snapshot; specification oracle/pyref/lasso.py and
//! oracle/pyref/hyperplonk.py LassoLookup).  NEVER COMPILED - see README.md.
use crate::{device::*, pcs::*, sys::*, transcript};
use halo2_curves::bn256::{Bn256, Fr, G1Affine};
use halo2_curves::ff::Field;
use plonkish_backend::{pcs::multilinear::MultilinearKzgVerifierParams, util::transcript::{TranscriptRead, TranscriptWrite}, Error};

fn table(num_chunks: u32, chunk_bits: u32, kind: u32, shift_bits: u32) -> lh_lasso_table {
    let mut t: lh_lasso_table = unsafe { std::mem::zeroed() };
    t.num_chunks = num_chunks;
    t.chunk_bits = chunk_bits;
    t.num_memories = num_chunks;
    t.num_terms = num_chunks;
    for j in 0..num_chunks as usize {
        t.memory_chunk[j] = j as u32;
        t.memory_subtable[j] = kind;
        // g = sum_j 2^(shift_bits * j) * E_j
        t.g_coeff[j] = Fr::from(2).pow([(shift_bits as u64) * j as u64]);
        t.g_num_factors[j] = 1;
        t.g_factor[j][0] = j as u8;
    }
    t
}
/// value < 2^(c*l): limbs looked up in the identity subtable (oracle/pyref/lasso.py range_table)
pub fn range_table(num_chunks: u32, chunk_bits: u32) -> lh_lasso_table {
    table(num_chunks, chunk_bits, LH_SUBTABLE_IDENTITY, chunk_bits)
}
/// AND / XOR of two (c*l/2)-bit operands, chunk j = x_j || y_j (oracle/pyref/lasso.py bitwise_table)
pub fn bitwise_table(xor: bool, num_chunks: u32, chunk_bits: u32) -> lh_lasso_table {
    table(num_chunks, chunk_bits, if xor { LH_SUBTABLE_XOR } else { LH_SUBTABLE_AND }, chunk_bits / 2)
}
/// OR of two (c*l/2)-bit operands (the bitwise table over LH_SUBTABLE_OR)
pub fn or_table(num_chunks: u32, chunk_bits: u32) -> lh_lasso_table {
    table(num_chunks, chunk_bits, LH_SUBTABLE_OR, chunk_bits / 2)
}
/// x == y for two (c*l/2)-bit operands, chunk 0 least significant: g = prod_j EQ_j.  None unless 1 <= c <= LH_SC_MAX_FACTORS.
pub fn equal_table(num_chunks: u32, chunk_bits: u32) -> Option<lh_lasso_table> {
    let c = num_chunks as usize;
    if c < 1 || c > LH_SC_MAX_FACTORS {
        return None;
    }
    let mut t: lh_lasso_table = unsafe { std::mem::zeroed() };
    t.num_chunks = num_chunks;
    t.chunk_bits = chunk_bits;
    t.num_memories = num_chunks;
    t.num_terms = 1;
    t.g_coeff[0] = Fr::ONE;
    t.g_num_factors[0] = c as u8;
    for j in 0..c {
        t.memory_chunk[j] = j as u32;
        t.memory_subtable[j] = LH_SUBTABLE_EQ;
        t.g_factor[0][j] = j as u8;
    }
    Some(t)
}
/// x < y (unsigned): memories LTU_0..LTU_{c-1}, EQ_1..EQ_{c-1}; g = sum_j LTU_j prod_{k > j} EQ_k.  None unless
/// 1 <= c <= LH_SC_MAX_FACTORS (c = 4, l = 16: 32-bit operands).
pub fn less_than_table(num_chunks: u32, chunk_bits: u32) -> Option<lh_lasso_table> {
    let c = num_chunks as usize;
    if c < 1 || c > LH_SC_MAX_FACTORS {
        return None;
    }
    let mut t: lh_lasso_table = unsafe { std::mem::zeroed() };
    t.num_chunks = num_chunks;
    t.chunk_bits = chunk_bits;
    t.num_memories = (2 * c - 1) as u32;
    t.num_terms = num_chunks;
    for j in 0..c {
        t.memory_chunk[j] = j as u32;
        t.memory_subtable[j] = LH_SUBTABLE_LTU;
        if j >= 1 {
            t.memory_chunk[c + j - 1] = j as u32;
            t.memory_subtable[c + j - 1] = LH_SUBTABLE_EQ;
        }
        t.g_coeff[j] = Fr::ONE;
        t.g_num_factors[j] = (c - j) as u8;
        t.g_factor[j][0] = j as u8;
        for k in (j + 1)..c {
            t.g_factor[j][k - j] = (c + k - 1) as u8;
        }
    }
    Some(t)
}

/// A caller-registered subtable (lh_subtable_register): 2^chunk_bits 32-bit entries, chunk_bits <= LH_SUBTABLE_CUSTOM_MAX_BITS.
/// The registry is process-wide and needs no ctx; `kind()` is what `lh_lasso_table::memory_subtable` names.  Kinds are never
/// reused: once the `Subtable` is dropped its kind is refused (LH_ERR_ARG).  A prove or verify that has looked the table up
/// keeps its entries alive.
pub struct Subtable {
    kind: u32,
    chunk_bits: u32,
    value_bits: u32,
    digest: [u8; 32],
}
impl Subtable {
    /// `values.len()` must be 2^chunk_bits with 1 <= chunk_bits <= LH_SUBTABLE_CUSTOM_MAX_BITS
    pub fn register(values: &[u32]) -> Result<Self, Error> {
        let n = values.len();
        if n < 2 || !n.is_power_of_two() {
            check(LH_ERR_ARG)?; // (the library reads 2^chunk_bits values: the length must be that)
        }
        let mut t = Subtable { kind: 0, chunk_bits: 0, value_bits: 0, digest: [0; 32] };
        check(unsafe { lh_subtable_register(values.as_ptr(), n.trailing_zeros(), &mut t.kind) })?;
        check(unsafe { lh_subtable_info(t.kind, &mut t.chunk_bits, &mut t.value_bits, t.digest.as_mut_ptr()) })?;
        Ok(t)
    }
    pub fn kind(&self) -> u32 { self.kind }
    pub fn chunk_bits(&self) -> u32 { self.chunk_bits }
    /// bit length of the largest entry (0: an all-zero table)
    pub fn value_bits(&self) -> u32 { self.value_bits }
    /// Keccak-256 of the entries as little-endian words: for comparing registrations across hosts, in no transcript
    pub fn digest(&self) -> &[u8; 32] { &self.digest }
}
impl Drop for Subtable {
    fn drop(&mut self) {
        unsafe { lh_subtable_unregister(self.kind) };
    }
}
/// one memory per chunk into the registered subtable, g = sum_j 2^(shift_bits * j) * E_j (the shape of the bitwise tables)
pub fn custom_table(subtable: &Subtable, num_chunks: u32, shift_bits: u32) -> lh_lasso_table {
    table(num_chunks, subtable.chunk_bits(), subtable.kind(), shift_bits)
}

/// dims[j]: chunk indices (< 2^chunk_bits) of every lookup, 2^num_vars entries each
pub fn prove(pp: &HipProverParam, table: &lh_lasso_table, num_vars: usize, dims: &[DeviceVec<u32>],
             transcript: &mut impl TranscriptWrite<G1Affine, Fr>) -> Result<(), Error> {
    let ptrs: Vec<*const u32> = dims.iter().map(|d| d.as_ptr()).collect();
    let mut vt = transcript::writer(transcript);
    check(unsafe { lh_lasso_prove(pp.ctx().raw(), pp.srs(), table, num_vars, ptrs.as_ptr(), &mut vt) })
}

pub fn verify(vp: &MultilinearKzgVerifierParams<Bn256>, table: &lh_lasso_table, num_vars: usize,
              transcript: &mut impl TranscriptRead<G1Affine, Fr>) -> Result<(), Error> {
    let h = vp_handle(vp)?;
    let mut vt = transcript::reader(transcript);
    check(unsafe { lh_lasso_verify(h.0, table, num_vars, &mut vt) })
}

/// A lookup of a HyperPlonk circuit proven by Lasso instead of LogUp: fill `lh_hp_param::lasso_lookups` /
/// `lh_hp_vparam::lasso_lookups` with these (backend.rs builds both structs; `PlonkishCircuitInfo` has no field for
/// it, so a circuit declares its Lasso lookups next to the info it hands to `preprocess`).
pub fn hp_lookup(table: lh_lasso_table, output_poly: usize, chunk_polys: &[usize]) -> lh_hp_lasso_lookup {
    let mut lk = lh_hp_lasso_lookup { table, output_poly, chunk_polys: [0; LH_LASSO_MAX_CHUNKS] };
    lk.chunk_polys[..chunk_polys.len()].copy_from_slice(chunk_polys);
    lk
}
