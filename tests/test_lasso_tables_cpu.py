"""CPU: the OR / EQ / LTU subtables and the less_than / equal tables - the reference extension (tests/lasso_tables_ref.py)
against brute force, and the product's host verifier (liblasso_hip.so, no GPU) against golden proofs made by the extended
Python oracle (tests/golden/lasso_tables.json, tests/golden/make_golden_lasso_tables.py)."""
import json
import os
import random

import pytest

import lasso_tables_ref as ltr
from oracle.pyref import lasso as o_lasso
from oracle.pyref.field import R_MOD as P
from oracle.pyref.poly import evaluate

GOLDEN = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "lasso_tables.json")))
SS = [int(x, 16) for x in GOLDEN["srs"]["ss"]]


@pytest.fixture
def tables_ref():
    with ltr.installed():
        yield ltr
    assert o_lasso.subtable_entry is not ltr.subtable_entry  # (the originals are back)


@pytest.fixture(scope="module")
def vp(hl):
    return hl.MultilinearKzgVerifierParams.setup(SS)


@pytest.mark.parametrize("l", [2, 4, 6])
@pytest.mark.parametrize("kind", ltr.NEW_KINDS)
def test_reference_mle_is_the_mle_of_the_entries(tables_ref, kind, l):
    rng = random.Random(100 * kind + l)
    table = [o_lasso.subtable_entry(kind, m, l) for m in range(1 << l)]
    for _ in range(4):
        point = [rng.randrange(P) for _ in range(l)]
        assert o_lasso.subtable_mle_eval(kind, point) == evaluate(table, point)
    for m in (0, 1, (1 << l) - 1, rng.randrange(1 << l)):  # on the cube: the entries themselves
        assert o_lasso.subtable_mle_eval(kind, [(m >> i) & 1 for i in range(l)]) == table[m]


def test_wrappers_delegate_the_old_kinds(tables_ref):
    for kind in (o_lasso.SUBTABLE_IDENTITY, o_lasso.SUBTABLE_AND, o_lasso.SUBTABLE_XOR):
        for m in range(16):
            assert o_lasso.subtable_entry(kind, m, 4) == ltr._ORIG_ENTRY(kind, m, 4)
        assert o_lasso.subtable_mle_eval(kind, [3, 5, 7, 11]) == ltr._ORIG_MLE(kind, [3, 5, 7, 11])
    with pytest.raises(ValueError):
        o_lasso.subtable_entry(6, 0, 4)


@pytest.mark.parametrize("c,l,n", [(4, 4, 6), (2, 4, 5), (1, 2, 1), (3, 6, 4), (4, 2, 3)])
def test_witness_is_the_integer_comparison(tables_ref, c, l, n):
    rng = random.Random(c * 100 + l * 10 + n)
    dims = [[rng.randrange(1 << l) for _ in range(1 << n)] for _ in range(c)]
    for k in range(0, 1 << n, 3):  # equal operands in a third of the lookups
        for j in range(c):
            dims[j][k] = (dims[j][k] >> (l // 2)) * ((1 << (l // 2)) + 1)
    xs, ys = ltr.operands(dims, l)
    assert o_lasso.witness(ltr.less_than_table(c, l), dims)["a"] == [int(x < y) for x, y in zip(xs, ys)]
    assert o_lasso.witness(ltr.equal_table(c, l), dims)["a"] == [int(x == y) for x, y in zip(xs, ys)]
    assert o_lasso.witness(ltr.or_table(c, l), dims)["a"] == [x | y for x, y in zip(xs, ys)]
    assert any(x == y for x, y in zip(xs, ys)) and any(x < y for x, y in zip(xs, ys))


def test_constructors_match_the_reference_specs(hl):
    for kind, c, l in (("or", 3, 4), ("equal", 4, 2), ("less_than", 4, 4), ("less_than", 1, 2)):
        spec, table = ltr.spec_of(kind, c, l), ltr.table_of(hl, kind, c, l)
        assert (table.c, table.l, table.memories) == (spec.c, spec.l, spec.memories)
        assert [(co, tuple(f)) for co, f in table.g_terms] == spec.g_terms
    assert (hl.SUBTABLE_OR, hl.SUBTABLE_EQ, hl.SUBTABLE_LTU) == ltr.NEW_KINDS
    assert len(hl.LassoTable.less_than(4, 16).memories) == 7


@pytest.mark.parametrize("idx", range(len(GOLDEN["lasso"])))
def test_golden_proofs_come_from_the_oracle(tables_ref, idx):
    """the committed vectors are what the generator makes: the oracle's own verifier accepts them, and `a` is the table"""
    from oracle.pyref import kzg as o_kzg
    from oracle.pyref.transcript import Keccak256Transcript as OT
    g = GOLDEN["lasso"][idx]
    o_lasso.verify(o_kzg.setup(SS), ltr.spec_of(g["kind"], g["c"], g["l"]), g["n"], OT(bytes.fromhex(g["proof"])))


@pytest.mark.parametrize("idx", range(len(GOLDEN["lasso"])))
def test_host_verifier_accepts_golden_and_rejects_flipped_bytes(hl, vp, idx):
    g = GOLDEN["lasso"][idx]
    table = ltr.table_of(hl, g["kind"], g["c"], g["l"])
    proof = bytes.fromhex(g["proof"])
    hl.lasso_verify(vp, table, g["n"], hl.Keccak256Transcript.from_proof(proof))
    rng = random.Random(idx)
    for _ in range(12):
        bad = bytearray(proof)
        bad[rng.randrange(len(bad))] ^= 1 << rng.randrange(8)
        with pytest.raises(hl.Error):
            hl.lasso_verify(vp, table, g["n"], hl.Keccak256Transcript.from_proof(bytes(bad)))


def test_less_than_proof_is_not_an_equal_proof(hl, vp):
    for g in GOLDEN["lasso"]:
        if g["kind"] != "less_than":
            continue
        with pytest.raises(hl.Error):
            hl.lasso_verify(vp, hl.LassoTable.equal(g["c"], g["l"]), g["n"],
                            hl.Keccak256Transcript.from_proof(bytes.fromhex(g["proof"])))
        # the same memories and g, one LTU subtable read as EQ: the memory-checking leaves no longer fit
        wrong = hl.LassoTable.less_than(g["c"], g["l"])
        wrong.memories[0] = (0, hl.SUBTABLE_EQ)
        with pytest.raises(hl.InvalidSnark):
            hl.lasso_verify(vp, wrong, g["n"], hl.Keccak256Transcript.from_proof(bytes.fromhex(g["proof"])))


def test_unknown_kind_and_too_many_chunks_are_argument_errors(hl, vp):
    g = GOLDEN["lasso"][0]
    bad = hl.LassoTable(g["c"], g["l"], [(j, 6) for j in range(g["c"])], [(1, [j]) for j in range(g["c"])])
    with pytest.raises(hl.ArgumentError):
        hl.lasso_verify(vp, bad, g["n"], hl.Keccak256Transcript.from_proof(bytes.fromhex(g["proof"])))
    with pytest.raises(hl.ArgumentError):  # refused before the prover param or the device is touched
        hl.lasso_prove(None, bad, g["n"], [None] * g["c"], hl.Keccak256Transcript())
    # the library's own check (not only the Python side's): the C table with kind 6 straight to the entry point
    import ctypes as C
    from halo2_lasso_amd import _ffi
    t = hl.LassoTable.bitwise(hl.SUBTABLE_OR, g["c"], g["l"]).to_c()
    t.memory_subtable[0] = 6
    tr = hl.Keccak256Transcript.from_proof(bytes.fromhex(g["proof"]))
    assert _ffi.load().lh_lasso_verify(*vp.head(), C.byref(t), g["n"], tr.p) == _ffi.LH_ERR_ARG
    with pytest.raises(hl.ArgumentError):
        hl.LassoTable.less_than(5, 4)
    with pytest.raises(hl.ArgumentError):
        hl.LassoTable.equal(5, 4)
    assert hl.LassoTable.less_than(4, 4).to_c().num_memories == 7
