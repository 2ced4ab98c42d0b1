"""CPU: the library's host verifier of Lasso over Hyrax (lh_lasso_verify_hyrax) against proofs made by the Python restatement
(tests/hyrax_provers_ref.py) on the issue's four inputs: acceptance with the transcript fully consumed, rejection of one flipped
bit in a mask, a row commitment, the claimed evaluation, a sum-check message and the opening, the "commitment mask out of
range" error, the size errors and the null arguments of the new entries.  The xor case has 72 points: two masks, so its
acceptance is the agreement of the C framing with the restated one on the two-mask case.  Then lh_hyperplonk_verify_hyrax on
proofs made by the oracle (oracle/pyref/hyperplonk.py) over the Hyrax restatement, and hyperplonk.batch_size."""
import ctypes as C

import pytest

import halo2_lasso_amd as hl
from halo2_lasso_amd import _ffi
import hyrax_provers_ref as hr


def _table(kind, c, l):
    return hl.LassoTable.range(c, l) if kind == "range" else hl.LassoTable.bitwise(
        hl.SUBTABLE_AND if kind == "and" else hl.SUBTABLE_XOR, c, l)


def _vp(case):
    kind, c, l, n, batch_size = case
    nv = max(n, l)
    return hl.Hyrax.trim(hl.Hyrax.setup(None, 1 << nv, batch_size), 1 << nv, batch_size)


def _layout(case):
    """byte offsets in the proof: (masks, first point, the claimed evaluation v, first sum-check message, opening tail)"""
    chunks, points, identities, masks, size = hr.LASSO_SHAPES[case]
    v = 32 * masks + 64 * (points - identities)
    return 0, 32 * masks, v, v + 32, size - 40


@pytest.mark.parametrize("case", hr.LASSO_CASES, ids=lambda c: "%s-%d-%d-%d-%d" % c)
def test_host_verifier_accepts_the_restatement_and_rejects_flipped_bits(case):
    kind, c, l, n, _ = case
    proof, flat = hr.lasso_proof(case)
    chunks, points, identities, masks, size = hr.LASSO_SHAPES[case]
    assert (len(flat), sum(p is None for p in flat), len(proof)) == (points, identities, size)
    vp, table = _vp(case), _table(kind, c, l)
    assert vp.num_chunks == chunks
    t = hl.Keccak256Transcript.from_proof(proof)
    hl.lasso_verify(vp, table, n, t)
    assert t.remaining() == 0
    for off in _layout(case):
        bad = bytearray(proof)
        bad[off + 30] ^= 4  # (a low byte of the field element, or a byte of the point's x)
        with pytest.raises(hl.Error):
            hl.lasso_verify(vp, table, n, hl.Keccak256Transcript.from_proof(bytes(bad)))
    with pytest.raises(hl.Error):
        hl.lasso_verify(vp, table, n, hl.Keccak256Transcript.from_proof(proof + bytes(32)))


@pytest.mark.parametrize("case,mask,bit", [(hr.LASSO_CASES[0], 0, 36), (hr.LASSO_CASES[0], 0, 62), (hr.LASSO_CASES[2], 1, 9),
                                           (hr.LASSO_CASES[2], 0, 63), (hr.LASSO_CASES[2], 1, 200)])
def test_a_mask_bit_beyond_its_width_is_out_of_range(case, mask, bit):
    """36 points: one mask of width 36; 72 points: widths 63 and 9"""
    kind, c, l, n, _ = case
    proof, _ = hr.lasso_proof(case)
    bad = bytearray(proof)
    bad[32 * mask + 31 - bit // 8] |= 1 << (bit % 8)  # (field elements cross the transcript most significant byte first)
    with pytest.raises(hl.InvalidSnark, match="commitment mask out of range"):
        hl.lasso_verify(_vp(case), _table(kind, c, l), n, hl.Keccak256Transcript.from_proof(bytes(bad)))


def test_restated_framing_reads_what_it_writes_and_equals_the_oracle_for_one_chunk():
    from oracle.pyref import lasso as o_lasso
    from oracle.pyref.transcript import Keccak256Transcript as OT
    from oracle.pyref import curve
    pts = [curve.mul(curve.G1_GEN, k + 2) for k in range(6)]
    comms = [[pts[0], None, pts[1]], [None, None, None], [pts[2], pts[3], None]] * 8  # 72 points, two masks
    a = OT()
    hr.write_commitments(a, comms)
    assert hr.read_commitments(OT(a.into_proof()), 24, 3) == comms
    one = [[p] for p in (pts[0], None, pts[4], None, pts[5])]
    a, b = OT(), OT()
    hr.write_commitments(a, one), o_lasso.write_commitments(b, [cm[0] for cm in one])
    assert a.into_proof() == b.into_proof()


def test_size_errors_and_null_arguments():
    case = hr.LASSO_CASES[0]
    kind, c, l, n, _ = case
    proof, _ = hr.lasso_proof(case)
    table = _table(kind, c, l)
    # a param of another size: max(n, l) = 4 is not its num_vars
    big = hl.Hyrax.trim(hl.Hyrax.setup(None, 1 << 6, 1), 1 << 6, 1)
    with pytest.raises(hl.ArgumentError, match="must equal log2"):
        hl.lasso_verify(big, table, n, hl.Keccak256Transcript.from_proof(proof))
    # a param whose rows are too short for the trim size
    short = hl.Hyrax.setup(None, 1 << 2, 1)
    lib, tc = _ffi.load(), table.to_c()
    t = hl.Keccak256Transcript.from_proof(proof)
    assert lib.lh_lasso_verify_hyrax(short.h, 1 << 6, 1, C.byref(tc), n, t.p) == _ffi.LH_ERR_INVALID_PCS_PARAM
    assert b"Too many variates to trim" in lib.lh_last_error()
    vp = _vp(case)
    bad = [lib.lh_lasso_verify_hyrax(None, 16, 1, C.byref(tc), n, t.p), lib.lh_lasso_verify_hyrax(vp.params.h, 16, 1, None, n, t.p),
           lib.lh_lasso_prove_hyrax(None, vp.params.h, 16, 1, C.byref(tc), n, None, t.p)]
    assert bad == [_ffi.LH_ERR_ARG] * 3


# ------------------------------------------------------------------ HyperPlonk over Hyrax
def _hp_vp(case, g_info, o_pp):
    """the library's verifier param with the commitments of the oracle's preprocess (num_chunks points per poly)"""
    from halo2_lasso_amd import hyperplonk as g_hp
    num_vars, batch_size = case[0], case[1]
    vp = g_hp.HyperPlonkVerifierParam()
    vp.pcs = hl.Hyrax.trim(hl.Hyrax.setup(None, 1 << num_vars, batch_size), 1 << num_vars, batch_size)
    vp.num_vars, vp.info = num_vars, g_info
    vp.num_permutation_z_polys, vp.expression = g_hp.compose(g_info)
    vp.preprocess_comms, vp.permutation_comms = o_pp.preprocess_comms, o_pp.permutation_comms
    return vp


def _g_info(case, o_info, instances):
    from halo2_lasso_amd import hyperplonk as g_hp
    mk = g_hp.vanilla_plonk_with_lookup_circuit_info if case[2] else g_hp.vanilla_plonk_circuit_info
    return mk(case[0], len(instances[0]), o_info.preprocess_polys, o_info.permutations)


@pytest.mark.parametrize("case", hr.HP_CASES, ids=lambda c: "%d-%d-%s-%d" % c)
def test_hyperplonk_host_verifier_accepts_the_oracle_over_hyrax(case):
    from halo2_lasso_amd import hyperplonk as g_hp
    o_info, instances, _, o_pp, proof = hr.hp_case(case)
    chunks, size = hr.HP_SHAPES[case]
    assert (o_pp.pcs.num_chunks, len(proof)) == (chunks, size)
    vp = _hp_vp(case, _g_info(case, o_info, instances), o_pp)
    assert vp.pcs.num_chunks == chunks and all(len(cm) == chunks for cm in vp.preprocess_comms + vp.permutation_comms)
    t = hl.Keccak256Transcript.from_proof(proof)
    g_hp.HyperPlonk.verify(vp, instances, t)
    assert t.remaining() == 0
    # a row commitment (the second point of the first witness commitment), a sum-check message, an evaluation, the opening
    for pos in (64 + 30, len(proof) // 3, len(proof) // 2, len(proof) - 40):
        bad = bytearray(proof)
        bad[pos] ^= 1
        with pytest.raises(hl.Error):
            g_hp.HyperPlonk.verify(vp, instances, hl.Keccak256Transcript.from_proof(bytes(bad)))
    with pytest.raises(hl.Error):
        g_hp.HyperPlonk.verify(vp, [[v + 1 for v in instances[0]]], hl.Keccak256Transcript.from_proof(proof))
    wrong = list(vp.preprocess_comms)
    wrong[0] = list(wrong[0][1:]) + [wrong[0][0]]  # the rows of one preprocess commitment rotated
    vp.preprocess_comms = wrong
    with pytest.raises(hl.Error):
        g_hp.HyperPlonk.verify(vp, instances, hl.Keccak256Transcript.from_proof(proof))


def test_hyperplonk_with_a_lasso_lookup_over_hyrax(monkeypatch):
    """the oracle's HyperPlonk frames its Lasso lookup's commitments through oracle.pyref.lasso: patched to the chunked
    framing for the length of this test"""
    import random
    from halo2_lasso_amd import hyperplonk as g_hp
    from oracle.pyref import hyperplonk as o_hp
    from oracle.pyref.transcript import Keccak256Transcript as OT
    from test_verifier import _lasso_circuit
    num_vars, case = 5, (5, 1, True, 0)
    # (xor, seed 1: the lookup's own witness columns have no all-zero row of 8 - most seeds give one, and a plainly written
    # witness commitment with an identity row ends the proof: tests/test_gpu_hyrax_provers.py)
    o_info, g_info, instances, witness = _lasso_circuit(hl, "xor", 2, 4, num_vars, 1)
    pp, _ = hr.params(num_vars, 1)
    hr.patch_lasso_framing(monkeypatch, pp.num_chunks)
    o_pp = o_hp.preprocess((pp, pp), o_info, hr.HyraxPcs)
    ot = OT()
    o_hp.prove(o_pp, instances, lambda r, ch: witness, ot)
    proof = ot.into_proof()
    o_hp.verify(o_pp, instances, hr.chunked_transcript(pp.num_chunks)(proof))
    vp = _hp_vp(case, g_info, o_pp)
    t = hl.Keccak256Transcript.from_proof(proof)
    g_hp.HyperPlonk.verify(vp, instances, t)
    assert t.remaining() == 0
    for pos in (len(proof) // 3, len(proof) // 2, len(proof) - 40):
        bad = bytearray(proof)
        bad[pos] ^= 1
        with pytest.raises(hl.Error):
            g_hp.HyperPlonk.verify(vp, instances, hl.Keccak256Transcript.from_proof(bytes(bad)))


def test_batch_size_restates_the_preprocessor():
    """preprocessor.rs:13-23: (preprocess + permutation polys) + sum of witness polys + lookups + (lookups +
    ceil(permutation polys / (max_degree - 1))).
    vanilla: 5 selectors, 3 witness polys that are all permuted, no lookup, max_degree 4 (the circuit info's own):
        (5 + 3) + 3 + 0 + (0 + ceil(3 / 3)) = 12
    vanilla with lookup: 5 selectors + q_lookup + 3 table columns = 9 preprocess polys, one lookup, max_degree 4 (the lookup's
    h (input + gamma)(table + gamma) with a degree-2 input):
        (9 + 3) + 3 + 1 + (1 + ceil(3 / 3)) = 18"""
    from halo2_lasso_amd import hyperplonk as g_hp
    for case, want in ((hr.HP_CASES[0], 12), (hr.HP_CASES[1], 18)):
        o_info, instances, _, _, _ = hr.hp_case(case)
        assert g_hp.batch_size(_g_info(case, o_info, instances)) == want


def test_hyperplonk_entries_sizes_and_null_arguments():
    from halo2_lasso_amd import hyperplonk as g_hp
    case = hr.HP_CASES[0]
    o_info, instances, _, o_pp, proof = hr.hp_case(case)
    g_info = _g_info(case, o_info, instances)
    vp = _hp_vp(case, g_info, o_pp)
    vp.pcs = hl.Hyrax.trim(hl.Hyrax.setup(None, 1 << 7, 1), 1 << 7, 1)  # a param of another size than the circuit
    with pytest.raises(hl.ArgumentError, match="must equal log2"):
        g_hp.HyperPlonk.verify(vp, instances, hl.Keccak256Transcript.from_proof(proof))
    lib = _ffi.load()
    t = hl.Keccak256Transcript.from_proof(proof)
    prm = _ffi.lh_hp_vparam()
    h = vp.pcs.params.h
    short = hl.Hyrax.setup(None, 1 << 2, 1)
    assert lib.lh_hyperplonk_verify_hyrax(short.h, 1 << 7, 1, C.byref(prm), None, t.p) == _ffi.LH_ERR_INVALID_PCS_PARAM
    assert b"Too many variates to trim" in lib.lh_last_error()
    one = (C.c_size_t * 1)(1)
    bad = [lib.lh_hyperplonk_verify_hyrax(None, 32, 1, C.byref(prm), None, t.p),
           lib.lh_hyperplonk_verify_hyrax(h, 32, 1, None, None, t.p),
           lib.lh_hyperplonk_verify_phases_hyrax(None, 32, 1, C.byref(prm), 1, one, one, None, t.p),
           lib.lh_hyperplonk_verify_phases_hyrax(h, 32, 1, None, 1, one, one, None, t.p),
           lib.lh_hyperplonk_verify_phases_hyrax(h, 32, 1, C.byref(prm), 1, None, one, None, t.p),
           lib.lh_hyperplonk_prove_hyrax(None, h, 32, 1, None, None, None, t.p),
           lib.lh_hyperplonk_prove_phases_hyrax(None, h, 32, 1, None, 1, one, one, None, None, t.p)]
    assert bad == [_ffi.LH_ERR_ARG] * len(bad)
