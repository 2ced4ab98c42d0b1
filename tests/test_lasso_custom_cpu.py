"""CPU: caller-registered subtables (lh_subtable_register, hl.Subtable) - the registry, the host verifier's MLE of the registered
entries against golden proofs made by the Python oracle extended by tests/lasso_custom_ref.py (tests/golden/lasso_custom.json,
tests/golden/make_lasso_custom.py), a built-in table registered as a custom one, and less_than_signed as integer comparison.

Every test closes what it registers: the only registrations that stay are less_than_signed's cached subtables."""
import ctypes as C
import json
import os
import random

import pytest

import lasso_custom_ref as lcr
import lasso_tables_ref as ltr
from oracle.pyref import kzg as o_kzg, lasso as o_lasso
from oracle.pyref.keccak import keccak256
from oracle.pyref.transcript import Keccak256Transcript as OT

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "lasso_custom.json")))
SS = [int(x, 16) for x in json.load(open(os.path.join(HERE, "golden", "lasso_tables.json")))["srs"]["ss"]]
VECTORS = json.load(open(os.path.join(HERE, "golden", "vectors.json")))


@pytest.fixture(scope="module")
def vp(hl):
    return hl.MultilinearKzgVerifierParams.setup(SS)


def _values(g):
    return lcr.lts_values(g["l"]) if g["table"] == "less_than_signed" else lcr.TABLES[g["table"]]


def _spec(g, kind):
    if g["table"] == "less_than_signed":
        return lcr.less_than_signed_spec(g["c"], g["l"], kind)
    return lcr.spec_of(g["table"], g["c"], g["g"], kind)


def _table(hl, g, kind):
    if g["table"] == "less_than_signed":
        return hl.LassoTable.less_than_signed(g["c"], g["l"])
    return lcr.table_of(hl, g["table"], g["c"], g["g"], kind)


# ------------------------------------------------------------------ 1. the registry
def test_register_info_unregister(hl):
    from halo2_lasso_amd import _ffi
    kinds = []
    for name, values in lcr.TABLES.items():
        with hl.Subtable.register(values) as t:
            assert t.kind >= _ffi.LH_SUBTABLE_CUSTOM_BASE == lcr.CUSTOM_BASE
            assert t.chunk_bits == lcr.bits_of(values)
            assert t.value_bits == max(values).bit_length(), name
            assert t.digest == keccak256(b"".join(v.to_bytes(4, "little") for v in values))
            assert int(t) == t.kind and hl.Subtable(t.kind).digest == t.digest
            kinds.append(t.kind)
        with pytest.raises(hl.ArgumentError):  # closed: the kind is gone
            hl.Subtable(kinds[-1])
    assert kinds == sorted(set(kinds)), "kinds only grow and are never reused"
    assert lcr.TABLES["zero"] == [0] * 4 and max(lcr.TABLES["wide"]) == (1 << 32) - 1  # (value_bits 0 and 32 were among them)
    again = hl.Subtable.register(lcr.TABLES["rand1"])
    assert again.kind > kinds[-1]
    again.close()
    again.close()  # (idempotent)


def test_refusals(hl):
    from halo2_lasso_amd import _ffi
    lib = _ffi.load()
    kind = C.c_uint32(7)
    two = (C.c_uint32 * 2)(0, 1)
    assert lib.lh_subtable_register(None, 1, C.byref(kind)) == _ffi.LH_ERR_ARG
    assert lib.lh_subtable_register(two, 1, None) == _ffi.LH_ERR_ARG
    assert lib.lh_subtable_register(two, 0, C.byref(kind)) == _ffi.LH_ERR_ARG
    assert lib.lh_subtable_register(two, _ffi.LH_SUBTABLE_CUSTOM_MAX_BITS + 1, C.byref(kind)) == _ffi.LH_ERR_ARG
    assert kind.value == 7 and lib.lh_last_error()  # untouched, and there is a message
    for unknown in (0, 5, 6, 0xFF, _ffi.LH_SUBTABLE_CUSTOM_BASE + (1 << 30)):
        assert lib.lh_subtable_unregister(unknown) == _ffi.LH_ERR_ARG
        assert lib.lh_subtable_info(unknown, None, None, None) == _ffi.LH_ERR_ARG
    for bad in ([], [1], [0, 1, 2], [0, 1 << 32], [0, -1]):
        with pytest.raises(hl.ArgumentError):
            hl.Subtable.register(bad)
    # the largest size registers (a 4 MB copy), and says so
    big = (C.c_uint32 * (1 << _ffi.LH_SUBTABLE_CUSTOM_MAX_BITS))()
    big[(1 << 20) - 1] = 5
    assert lib.lh_subtable_register(big, 20, C.byref(kind)) == _ffi.LH_OK
    t = hl.Subtable(kind.value)
    assert (t.chunk_bits, t.value_bits) == (20, 3)
    t.close()


def test_the_65th_registration_is_refused(hl):
    from halo2_lasso_amd import _ffi
    live = len(hl._LTS_SUBTABLES)  # (what stays registered in this process: see the module docstring)
    tables = []
    try:
        for _ in range(_ffi.LH_SUBTABLE_CUSTOM_MAX - live):
            tables.append(hl.Subtable.register([0, 1]))
        with pytest.raises(hl.ArgumentError):
            hl.Subtable.register([0, 1])
        tables.pop().close()
        tables.append(hl.Subtable.register([1, 0]))  # room again after one unregister
        with pytest.raises(hl.ArgumentError):
            hl.Subtable.register([0, 1])
    finally:
        for t in tables:
            t.close()


def test_stale_kind_and_wrong_chunk_bits_are_argument_errors(hl, vp):
    from halo2_lasso_amd import _ffi
    g = GOLDEN["lasso"][0]
    proof = bytes.fromhex(g["proof"])
    t = hl.Subtable.register(_values(g))
    table = _table(hl, g, t)
    tc = table.to_c()
    assert tc.memory_subtable[0] == t.kind
    wrong = table.to_c()
    wrong.chunk_bits = g["l"] + 1
    tr = hl.Keccak256Transcript.from_proof(proof)
    assert _ffi.load().lh_lasso_verify(*vp.head(), C.byref(wrong), g["n"], tr.p) == _ffi.LH_ERR_ARG
    with pytest.raises(hl.ArgumentError):
        hl.lasso_verify(vp, hl.LassoTable(g["c"], g["l"] + 1, table.memories, table.g_terms), g["n"],
                        hl.Keccak256Transcript.from_proof(proof))
    hl.lasso_verify(vp, table, g["n"], hl.Keccak256Transcript.from_proof(proof))
    stale = t.kind
    t.close()
    tr = hl.Keccak256Transcript.from_proof(proof)
    assert _ffi.load().lh_lasso_verify(*vp.head(), C.byref(tc), g["n"], tr.p) == _ffi.LH_ERR_ARG
    for memories in (table.memories, [(j, stale) for j in range(g["c"])]):
        with pytest.raises(hl.ArgumentError):
            hl.lasso_verify(vp, hl.LassoTable(g["c"], g["l"], memories, table.g_terms), g["n"],
                            hl.Keccak256Transcript.from_proof(proof))
    with pytest.raises(hl.ArgumentError):  # refused before the prover param or the device is touched
        hl.lasso_prove(None, hl.LassoTable(g["c"], g["l"], [(j, stale) for j in range(g["c"])], table.g_terms), g["n"],
                       [None] * g["c"], hl.Keccak256Transcript())
    # kinds 6 .. 0xFF keep their message
    with pytest.raises(hl.ArgumentError, match="unknown subtable"):
        hl.LassoTable(1, 2, [(0, 0xFF)], [(1, [0])]).check()


# ------------------------------------------------------------------ 2. the library's MLE is the MLE of the entries
def test_reference_extension(hl):
    rng = random.Random(5)
    tables = {lcr.CUSTOM_BASE + i: v for i, v in enumerate(lcr.TABLES.values())}
    with lcr.installed(tables):
        for kind, values in tables.items():
            l = lcr.bits_of(values)
            assert [o_lasso.subtable_entry(kind, m, l) for m in range(1 << l)] == values
            for m in (0, 1, (1 << l) - 1):  # on the cube: the entries themselves
                assert o_lasso.subtable_mle_eval(kind, [(m >> i) & 1 for i in range(l)]) == values[m]
        for kind in (0, 1, 2) + ltr.NEW_KINDS:  # everything else is delegated
            point = [rng.randrange(lcr.P) for _ in range(4)]
            assert o_lasso.subtable_mle_eval(kind, point) == ltr.subtable_mle_eval(kind, point)
            assert o_lasso.subtable_entry(kind, 9, 4) == ltr.subtable_entry(kind, 9, 4)
    assert o_lasso.subtable_entry is ltr._ORIG_ENTRY  # (the originals are back)
    assert lcr.TABLES["rand1"][0] == 0 and lcr.TABLES["rand1n"][0] == 1 and lcr.TABLES["wide"][0] == 0
    assert lcr.TABLES["lts"][0] == 0 and lcr.TABLES["and8"] == [ltr._ORIG_ENTRY(1, m, 8) for m in range(256)]


@pytest.mark.parametrize("idx", range(len(GOLDEN["lasso"])))
def test_golden_proofs_come_from_the_oracle(idx):
    g = GOLDEN["lasso"][idx]
    kind = lcr.CUSTOM_BASE + 3
    with lcr.installed({kind: _values(g)}):
        o_lasso.verify(o_kzg.setup(SS), _spec(g, kind), g["n"], OT(bytes.fromhex(g["proof"])))
    assert [(x["table"], x["c"], x["n"], x["g"]) for x in GOLDEN["lasso"][:4]] == lcr.CASES and len(GOLDEN["lasso"]) == 5


@pytest.mark.parametrize("idx", range(len(GOLDEN["lasso"])))
def test_host_verifier_accepts_golden_and_rejects_flipped_bytes(hl, vp, idx):
    g = GOLDEN["lasso"][idx]
    proof = bytes.fromhex(g["proof"])
    with hl.Subtable.register(_values(g)) as t:
        table = _table(hl, g, t)
        tr = hl.Keccak256Transcript.from_proof(proof)
        hl.lasso_verify(vp, table, g["n"], tr)
        assert tr.remaining() == 0
        rng = random.Random(idx)
        for _ in range(12):
            bad = bytearray(proof)
            bad[rng.randrange(len(bad))] ^= 1 << rng.randrange(8)
            with pytest.raises(hl.Error):
                hl.lasso_verify(vp, table, g["n"], hl.Keccak256Transcript.from_proof(bytes(bad)))


def test_a_proof_for_one_table_is_rejected_under_another(hl, vp):
    g = GOLDEN["lasso"][0]
    assert g["table"] == "rand1"
    with hl.Subtable.register(lcr.TABLES["rand1n"]) as t:
        with pytest.raises(hl.InvalidSnark):
            hl.lasso_verify(vp, _table(hl, g, t), g["n"], hl.Keccak256Transcript.from_proof(bytes.fromhex(g["proof"])))


# ------------------------------------------------------------------ 3. a built-in registered as custom is the built-in
def test_registered_and_entries_verify_the_builtin_and_proof(hl):
    g = next(g for g in VECTORS["lasso"] if g["kind"] == "and")
    vp5 = hl.MultilinearKzgVerifierParams.setup([int(x, 16) for x in VECTORS["srs"]["ss"]])
    proof = bytes.fromhex(g["proof"])
    c, l = g["c"], g["l"]
    entries = [o_lasso.subtable_entry(o_lasso.SUBTABLE_AND, m, l) for m in range(1 << l)]
    builtin = hl.LassoTable.bitwise(hl.SUBTABLE_AND, c, l)
    hl.lasso_verify(vp5, builtin, g["n"], hl.Keccak256Transcript.from_proof(proof))
    with hl.Subtable.register(entries) as t:
        custom = hl.LassoTable(c, l, [(j, t) for j in range(c)], builtin.g_terms)
        tr = hl.Keccak256Transcript.from_proof(proof)
        hl.lasso_verify(vp5, custom, g["n"], tr)
        assert tr.remaining() == 0
    with hl.Subtable.register([e ^ (m == 3) for m, e in enumerate(entries)]) as t:  # one entry off: no longer the AND table
        with pytest.raises(hl.InvalidSnark):
            hl.lasso_verify(vp5, hl.LassoTable(c, l, [(j, t) for j in range(c)], builtin.g_terms), g["n"],
                            hl.Keccak256Transcript.from_proof(proof))


# ------------------------------------------------------------------ 4. less_than_signed is integer comparison
@pytest.mark.parametrize("c,l,n", [(4, 4, 6), (2, 4, 5), (1, 2, 1)])
def test_less_than_signed_is_the_integer_comparison(hl, c, l, n):
    table = hl.LassoTable.less_than_signed(c, l)
    top = table.memories[c - 1][1]
    assert hl.LassoTable.less_than_signed(c, l).memories[c - 1][1] is top, "registered once per chunk_bits"
    assert (top.chunk_bits, top.value_bits) == (l, 1)
    spec = lcr.less_than_signed_spec(c, l, top.kind)
    assert (table.c, table.l, [(j, int(k)) for j, k in table.memories]) == (spec.c, spec.l, spec.memories)
    assert [(co, tuple(f)) for co, f in table.g_terms] == spec.g_terms
    unsigned = hl.LassoTable.less_than(c, l)
    assert [j for j, _ in table.memories] == [j for j, _ in unsigned.memories] and table.g_terms == unsigned.g_terms
    dims = lcr.comparison_dims(c, l, n)
    if n == 1:  # two lookups cannot hold an equal pair as well: (negative, non-negative) and (non-negative, negative)
        dims = [[1 << (l - 1), 1 << (l // 2 - 1)]]
    sx, sy = lcr.signed_operands(dims, l)
    with lcr.installed({top.kind: lcr.lts_values(l)}):
        a = o_lasso.witness(spec, dims)["a"]
    assert a == [int(x < y) for x, y in zip(sx, sy)]
    signs = {(x < 0, y < 0) for x, y in zip(sx, sy)}
    assert {(True, False), (False, True)} <= signs, "both mixed sign combinations are present"
    if n > 1:
        assert len(signs) == 4 and sum(x == y for x, y in zip(sx, sy)) >= len(sx) // 3
        assert 0 < sum(a) < len(a)


def test_less_than_signed_refusals(hl):
    with pytest.raises(hl.ArgumentError):
        hl.LassoTable.less_than_signed(5, 4)  # a term of five factors, as less_than(5, 4)
    with pytest.raises(hl.ArgumentError):
        hl.LassoTable.less_than_signed(2, 3)
    with pytest.raises(hl.ArgumentError):
        hl.LassoTable.less_than_signed(2, 22)
