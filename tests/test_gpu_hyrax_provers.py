"""GPU: Lasso over MultilinearHyrax (lh_lasso_prove_hyrax: Pcs::commit_columns over the row kernels of
csrc/kernels_hyrax.hip) against the Python restatement (tests/hyrax_provers_ref.py) byte for byte on the issue's four inputs,
through both verifiers, on both commit routes, and at size through the host verifier; then HyperPlonk over Hyrax
(lh_hyperplonk_prove[_phases]_hyrax) against the oracle (oracle/pyref/hyperplonk.py over the Hyrax restatement): preprocess and
permutation commitments, proof bytes, both verifiers, a two-phase circuit, a circuit with a Lasso lookup, and the identity-row
end.

What the shapes put under test:
  and (c 2, l 4, n 3)      n < l: every n-variable column has 8 entries in a table of 16 (4 rows of 4) - its rows 2 and 3 lie
                           beyond the column, launch no workgroup and come out as (0, 0): 16 identities under the mask
  xor (n 6)                8 rows of 8, 72 points: two masks
  range (n 6, batch 4)     rows of 16: batch_size changes the row length, not the table
  at size (l 8, n 14)      128 rows of 128: read_ts columns with real counts (bits from the counters' OR), and final_cts with 2^8
                           entries inside 2^14 - two live rows of 128, 126 rows that launch nothing
"""
import array
import ctypes as C
import random

import pytest

import hyrax_provers_ref as hr
from oracle.pyref.transcript import Keccak256Transcript as OT

pytestmark = pytest.mark.gpu


def _table(hl, kind, c, l):
    return hl.LassoTable.range(c, l) if kind == "range" else hl.LassoTable.bitwise(
        hl.SUBTABLE_AND if kind == "and" else hl.SUBTABLE_XOR, c, l)


def _params(hl, ctx, nv, batch_size):
    pp = hl.Hyrax.trim(hl.Hyrax.setup(ctx, 1 << nv, batch_size), 1 << nv, batch_size)
    return pp, hl.Hyrax.trim(hl.Hyrax.setup(None, 1 << nv, batch_size), 1 << nv, batch_size)


def _prove(hl, ctx, pp, table, n, dims):
    t = hl.Keccak256Transcript()
    hl.lasso_prove(pp, table, n, [ctx.upload(array.array("I", d).tobytes()) for d in dims], t)
    return t.into_proof()


@pytest.mark.parametrize("case", hr.LASSO_CASES, ids=lambda c: "%s-%d-%d-%d-%d" % c)
def test_lasso_over_hyrax_matches_the_restatement(hl, ctx, case):
    kind, c, l, n, batch_size = case
    spec, dims, _, o_vp = hr.lasso_case(*case)
    want, _ = hr.lasso_proof(case)
    pp, vp = _params(hl, ctx, max(n, l), batch_size)
    table = _table(hl, kind, c, l)
    proof = _prove(hl, ctx, pp, table, n, dims)
    assert proof == want and len(proof) == hr.LASSO_SHAPES[case][4]
    hr.verify(o_vp, spec, n, OT(proof))
    t = hl.Keccak256Transcript.from_proof(proof)
    hl.lasso_verify(vp, table, n, t)
    assert t.remaining() == 0
    bad = bytearray(proof)
    bad[len(bad) // 2] ^= 8
    with pytest.raises(hl.Error):
        hl.lasso_verify(vp, table, n, hl.Keccak256Transcript.from_proof(bytes(bad)))


def test_lasso_proof_is_the_same_on_both_commit_routes(hl, ctx):
    case = hr.LASSO_CASES[1]  # (the one with rows beyond its columns)
    kind, c, l, n, batch_size = case
    _, dims, _, _ = hr.lasso_case(*case)
    pp, _ = _params(hl, ctx, max(n, l), batch_size)
    proofs = []
    try:
        for route in (0, 1):
            hl.set_option(ctx, "hyrax_rows", route)
            proofs.append(_prove(hl, ctx, pp, _table(hl, kind, c, l), n, dims))
    finally:
        hl.set_option(ctx, "hyrax_rows", 1)
    assert proofs[0] == proofs[1] == hr.lasso_proof(case)[0]
    with pytest.raises(hl.ArgumentError):
        hl.set_option(ctx, "hyrax_rows", 2)


def test_lasso_over_hyrax_at_size_through_the_host_verifier(hl, ctx):
    c, l, n = 2, 8, 14
    rng = random.Random(714)
    dims = [[rng.randrange(1 << l) for _ in range(1 << n)] for _ in range(c)]
    pp, vp = _params(hl, ctx, n, 1)
    assert (pp.num_chunks, 1 << pp.row_num_vars) == (128, 128)
    table = _table(hl, "range", c, l)
    proof = _prove(hl, ctx, pp, table, n, dims)
    route = hl.lasso_last_route(ctx)
    assert route["derived_commitments"] == route["packed_ts_pairs"] == route["sorted_dim_reuse"] == 0
    t = hl.Keccak256Transcript.from_proof(proof)
    hl.lasso_verify(vp, table, n, t)
    assert t.remaining() == 0
    # (field elements cross the transcript most significant byte first) the commitments sit behind the masks: 9 commitments of 128 points, 19 masks; final_cts_j has rows 2.. as identities
    total, chunks = 9 * 128, 128
    masks = [int.from_bytes(proof[32 * k:32 * k + 32], "big") for k in range((total + 62) // 63)]
    ident = [(masks[i // 63] >> (i % 63)) & 1 for i in range(total)]
    for j in range(c):
        first = (1 + 2 * c + c + j) * chunks  # a, dim, read_ts, E (alpha = c), final_cts
        assert ident[first:first + chunks] == [0, 0] + [1] * (chunks - 2)
    assert sum(ident[:(1 + 2 * c + c) * chunks]) == 0


def test_sizes_and_null_arguments_of_the_prover_entry(hl, ctx):
    from halo2_lasso_amd import _ffi
    case = hr.LASSO_CASES[0]
    kind, c, l, n, _ = case
    _, dims, _, _ = hr.lasso_case(*case)
    table = _table(hl, kind, c, l)
    big, _ = _params(hl, ctx, 6, 1)
    with pytest.raises(hl.ArgumentError, match="must equal log2"):
        _prove(hl, ctx, big, table, n, dims)
    pp, _ = _params(hl, ctx, 4, 1)
    lib, tc, t = ctx.lib, table.to_c(), hl.Keccak256Transcript()
    bufs = [ctx.upload(array.array("I", d).tobytes()) for d in dims]
    ptrs = hl._ptr_array(bufs)
    bad = [lib.lh_lasso_prove_hyrax(None, pp.params.h, 16, 1, C.byref(tc), n, ptrs, t.p),
           lib.lh_lasso_prove_hyrax(ctx.h, None, 16, 1, C.byref(tc), n, ptrs, t.p),
           lib.lh_lasso_prove_hyrax(ctx.h, pp.params.h, 16, 1, None, n, ptrs, t.p),
           lib.lh_lasso_prove_hyrax(ctx.h, pp.params.h, 16, 1, C.byref(tc), n, None, t.p)]
    assert bad == [_ffi.LH_ERR_ARG] * 4
    assert lib.lh_lasso_prove_hyrax(ctx.h, pp.params.h, 1 << 10, 1, C.byref(tc), n, ptrs, t.p) == _ffi.LH_ERR_INVALID_PCS_PARAM
    host_only = hl.Hyrax.trim(hl.Hyrax.setup(None, 16, 1), 16, 1)
    host_only.ctx = ctx
    with pytest.raises(hl.ArgumentError, match="without a ctx"):
        _prove(hl, ctx, host_only, table, n, dims)


# ------------------------------------------------------------------ HyperPlonk over Hyrax
def _hp_params(hl, ctx, num_vars, batch_size):
    return _params(hl, ctx, num_vars, batch_size)


def _g_info(case, o_info, instances):
    from halo2_lasso_amd import hyperplonk as g_hp
    mk = g_hp.vanilla_plonk_with_lookup_circuit_info if case[2] else g_hp.vanilla_plonk_circuit_info
    return mk(case[0], len(instances[0]), o_info.preprocess_polys, o_info.permutations)


@pytest.mark.parametrize("case", hr.HP_CASES, ids=lambda c: "%d-%d-%s-%d" % c)
def test_hyperplonk_over_hyrax_matches_the_oracle(hl, ctx, case):
    from halo2_lasso_amd import hyperplonk as g_hp
    from oracle.pyref import hyperplonk as o_hp
    num_vars, batch_size = case[0], case[1]
    o_info, instances, witness, o_pp, want = hr.hp_case(case)
    pcs_pp, pcs_vp = _hp_params(hl, ctx, num_vars, batch_size)
    g_pp, g_vp = g_hp.HyperPlonk.preprocess(pcs_pp, _g_info(case, o_info, instances), pcs_vp)
    assert g_pp.preprocess_comms == o_pp.preprocess_comms and g_pp.permutation_comms == o_pp.permutation_comms
    t = hl.Keccak256Transcript()
    g_hp.HyperPlonk.prove(g_pp, instances, [hl.MultilinearPolynomial.new(ctx, w) for w in witness], t)
    proof = t.into_proof()
    assert proof == want and len(proof) == hr.HP_SHAPES[case][1]
    o_hp.verify(o_pp, instances, hr.chunked_transcript(pcs_pp.num_chunks)(proof))
    r = hl.Keccak256Transcript.from_proof(proof)
    g_hp.HyperPlonk.verify(g_vp, instances, r)
    assert r.remaining() == 0
    bad = bytearray(proof)
    bad[len(bad) // 2] ^= 8
    with pytest.raises(hl.Error):
        g_hp.HyperPlonk.verify(g_vp, instances, hl.Keccak256Transcript.from_proof(bytes(bad)))


def test_hyperplonk_prove_phases_over_hyrax(hl, ctx):
    from halo2_lasso_amd import hyperplonk as g_hp, expression as g_ex
    from oracle.pyref import hyperplonk as o_hp, expression as o_ex
    from test_gpu_hyperplonk import _two_phase_circuit
    num_vars = 5
    o_info, instances, o_synth = _two_phase_circuit(o_ex, o_hp.CircuitInfo, num_vars, random.Random(num_vars), None)
    g_info, _, _ = _two_phase_circuit(g_ex, g_hp.PlonkishCircuitInfo, num_vars, random.Random(num_vars), None)
    o_pp = o_hp.preprocess(hr.params(num_vars, 1), o_info, hr.HyraxPcs)
    ot = OT()
    o_hp.prove(o_pp, instances, o_synth, ot)
    pcs_pp, pcs_vp = _hp_params(hl, ctx, num_vars, 1)
    g_pp, g_vp = g_hp.HyperPlonk.preprocess(pcs_pp, g_info, pcs_vp)
    assert g_pp.preprocess_comms == o_pp.preprocess_comms  # (q_inst has all-zero rows: identities, never written)
    calls = []

    def synth(rnd, challenges):
        calls.append(rnd)
        return [hl.MultilinearPolynomial.new(ctx, w) for w in o_synth(rnd, challenges)]
    t = hl.Keccak256Transcript()
    g_hp.HyperPlonk.prove(g_pp, instances, synth, t)
    proof = t.into_proof()
    assert calls == [0, 1] and proof == ot.into_proof()
    r = hl.Keccak256Transcript.from_proof(proof)
    g_hp.HyperPlonk.verify(g_vp, instances, r)
    assert r.remaining() == 0


def test_hyperplonk_with_a_lasso_lookup_over_hyrax(hl, ctx, monkeypatch):
    from halo2_lasso_amd import hyperplonk as g_hp
    from oracle.pyref import hyperplonk as o_hp
    from test_verifier import _lasso_circuit
    num_vars = 5
    o_info, g_info, instances, witness = _lasso_circuit(hl, "xor", 2, 4, num_vars, 1)  # (no all-zero witness row: the CPU test)
    pp, _ = hr.params(num_vars, 1)
    hr.patch_lasso_framing(monkeypatch, pp.num_chunks)
    o_pp = o_hp.preprocess((pp, pp), o_info, hr.HyraxPcs)
    ot = OT()
    o_hp.prove(o_pp, instances, lambda r, ch: witness, ot)
    pcs_pp, pcs_vp = _hp_params(hl, ctx, num_vars, 1)
    g_pp, g_vp = g_hp.HyperPlonk.preprocess(pcs_pp, g_info, pcs_vp)
    t = hl.Keccak256Transcript()
    g_hp.HyperPlonk.prove(g_pp, instances, [hl.MultilinearPolynomial.new(ctx, w) for w in witness], t)
    proof = t.into_proof()
    assert proof == ot.into_proof()
    r = hl.Keccak256Transcript.from_proof(proof)
    g_hp.HyperPlonk.verify(g_vp, instances, r)
    assert r.remaining() == 0


def test_an_identity_row_of_a_witness_commitment_ends_the_proof_as_in_the_reference(hl, ctx):
    """the witness, m, h and z commitments are written plainly: a witness column whose second row (of 8) is all zero has an
    identity row commitment, which no transcript carries - TranscriptError on both sides after the same bytes (the first
    row's point)"""
    from halo2_lasso_amd import hyperplonk as g_hp
    from oracle.pyref import hyperplonk as o_hp
    from oracle.pyref.transcript import TranscriptError
    case = hr.HP_CASES[0]
    o_info, instances, witness, o_pp, _ = hr.hp_case(case)
    witness = [list(w) for w in witness]
    witness[0][8:16] = [0] * 8
    ot = OT()
    with pytest.raises(TranscriptError):
        o_hp.prove(o_pp, instances, lambda r, ch: witness, ot)
    pcs_pp, pcs_vp = _hp_params(hl, ctx, case[0], case[1])
    g_pp = g_hp.HyperPlonk.preprocess(pcs_pp, _g_info(case, o_info, instances))
    t = hl.Keccak256Transcript()
    with pytest.raises(hl.TranscriptError):
        g_hp.HyperPlonk.prove(g_pp, instances, [hl.MultilinearPolynomial.new(ctx, w) for w in witness], t)
    written = t.into_proof()
    assert written == ot.into_proof() and len(written) == 64


def test_null_arguments_of_the_hyperplonk_prover_entries(hl, ctx):
    from halo2_lasso_amd import _ffi
    pp, _ = _hp_params(hl, ctx, 5, 1)
    lib, h, p, t = ctx.lib, ctx.h, pp.params.h, hl.Keccak256Transcript()
    prm = _ffi.lh_hp_param()
    prm.num_witness_polys = 1
    circ = _ffi.lh_hp_circuit()
    bad = [lib.lh_hyperplonk_prove_hyrax(None, p, 32, 1, C.byref(prm), None, None, t.p),
           lib.lh_hyperplonk_prove_hyrax(h, None, 32, 1, C.byref(prm), None, None, t.p),
           lib.lh_hyperplonk_prove_hyrax(h, p, 32, 1, None, None, None, t.p),
           lib.lh_hyperplonk_prove_hyrax(h, p, 32, 1, C.byref(prm), None, None, t.p),
           lib.lh_hyperplonk_prove_phases_hyrax(None, p, 32, 1, C.byref(prm), 0, None, None, None, C.byref(circ), t.p),
           lib.lh_hyperplonk_prove_phases_hyrax(h, None, 32, 1, C.byref(prm), 0, None, None, None, C.byref(circ), t.p),
           lib.lh_hyperplonk_prove_phases_hyrax(h, p, 32, 1, None, 0, None, None, None, C.byref(circ), t.p),
           lib.lh_hyperplonk_prove_phases_hyrax(h, p, 32, 1, C.byref(prm), 0, None, None, None, None, t.p)]
    assert bad == [_ffi.LH_ERR_ARG] * len(bad)
