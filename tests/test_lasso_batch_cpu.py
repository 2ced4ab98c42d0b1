"""CPU: lookups into several tables in one proof (lh_lasso_prove_batch / lh_lasso_verify_batch) - the reference of the
protocol (tests/lasso_batch_ref.py) against itself and against its golden proofs (tests/golden/lasso_batch.json,
tests/golden/make_lasso_batch.py), the host verifier on those proofs and on damaged ones, and the argument refusals of both
entries that need no device."""
import ctypes as C
import json
import os

import pytest

import lasso_batch_ref as lbr
import lasso_custom_ref as lcr
from oracle.pyref import gkr as o_gkr, kzg as o_kzg, sum_check as o_sc
from oracle.pyref.transcript import Keccak256Transcript as OT

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "lasso_batch.json")))["cases"]
SS = [int(x, 16) for x in json.load(open(os.path.join(HERE, "golden", "lasso_tables.json")))["srs"]["ss"]]
CASES = list(lbr.CASES)


@pytest.fixture(scope="module")
def vp(hl):
    return hl.MultilinearKzgVerifierParams.setup(SS)


@pytest.fixture(scope="module")
def pp():
    return o_kzg.setup(SS)


def golden_dims(case):
    g = GOLDEN[case]
    return g["dims"] * len(lbr.CASES[case][1]) if case in lbr.SHARED else g["dims"]


def tables_of(hl, case, kind=None):
    return [lbr.table_of(hl, d, kind) for d in lbr.CASES[case][1]]


class registered:
    """the library's side of lasso_custom_ref.installed: registers the tables a case names, yields the kind (or None)"""

    def __init__(self, hl, case):
        values = list(lbr.custom_values(case).values())
        self.t = hl.Subtable.register(values[0]) if values else None

    def __enter__(self):
        return self.t

    def __exit__(self, *exc):
        if self.t is not None:
            self.t.close()


# ------------------------------------------------------------------ 1. the reference
def test_the_cases_are_the_named_ones():
    assert set(GOLDEN) == set(lbr.CASES) and len(lbr.CASES) == 8
    alphas = {case: sum(lbr.spec_of(d).alpha for d in descs) for case, (_, descs) in lbr.CASES.items()}
    assert alphas["two_ranges"] == 4 and alphas["mixed_g"] == 5 and alphas["full"] == 8
    n, descs = lbr.CASES["pad"]
    assert all(lbr.spec_of(d).l > n for d in descs)
    assert len({lbr.spec_of(d).l for d in lbr.CASES["two_ranges"][1]}) == 2
    dims = lbr.case_dims("and_xor_shared")
    assert dims[0] is dims[1]
    # zeros: the AND table's operands share no bit (E = 0 everywhere), the range's high chunk is all zero
    z = lbr.case_dims("zeros")
    assert all((m >> 2) & (m & 3) == 0 for d in z[0] for m in d) and not any(z[1][-1]) and any(z[1][0])


@pytest.mark.parametrize("case", CASES)
def test_reference_proves_verifies_and_matches_golden(pp, case):
    n, descs = lbr.CASES[case]
    specs = [lbr.spec_of(d) for d in descs]
    dims = lbr.case_dims(case)
    assert (dims[:1] if case in lbr.SHARED else dims) == GOLDEN[case]["dims"] and n == GOLDEN[case]["n"]
    with lcr.installed(lbr.custom_values(case)):
        t = OT()
        lbr.prove(pp, specs, dims, t)
        proof = t.into_proof()
        lbr.verify(pp, specs, n, OT(proof))
    assert proof.hex() == GOLDEN[case]["proof"], "the golden bytes are not what the reference produces now"


def test_a_table_block_is_its_single_proof_block(pp):
    """spec step 1: with the same nv, a table's commitment block is byte for byte the block of its own lasso.prove proof"""
    from oracle.pyref import lasso as o_lasso
    n, descs = lbr.CASES["full"]
    proof = bytes.fromhex(GOLDEN["full"]["proof"])
    at = 0
    for desc, dims in zip(descs, golden_dims("full")):
        t = OT()
        o_lasso.prove(pp, lbr.spec_of(desc), dims, t)
        single = t.into_proof()
        spec = lbr.spec_of(desc)
        size = _block_bytes(single, 1 + 3 * spec.c + spec.alpha)
        assert proof[at:at + size] == single[:size]
        at += size


def _block_bytes(stream, count):
    """bytes of a commitment block that starts `stream`: the mask element, then 64 per commitment that is not the identity"""
    mask = int.from_bytes(stream[:32], "little")
    assert mask >> count == 0
    return 32 + 64 * (count - bin(mask).count("1"))


# ------------------------------------------------------------------ 2. the host verifier
@pytest.mark.parametrize("case", CASES)
def test_host_verifier_accepts_golden(hl, vp, case):
    n = lbr.CASES[case][0]
    with registered(hl, case) as kind:
        tr = hl.Keccak256Transcript.from_proof(bytes.fromhex(GOLDEN[case]["proof"]))
        hl.lasso_verify_batch(vp, tables_of(hl, case, kind), n, tr)
        assert tr.remaining() == 0


def _sections(pp, case, monkeypatch):
    """where the sections of a golden proof begin: the reference's verifier is asked, at the entry of its pieces"""
    n, descs = lbr.CASES[case]
    at = {}

    def spy(name, fn, tr_arg):
        def wrapped(*a, **k):
            at.setdefault(name, a[tr_arg].pos)
            return fn(*a, **k)
        return wrapped

    monkeypatch.setattr(o_sc, "verify", spy("surge", o_sc.verify, 4))
    monkeypatch.setattr(o_gkr, "verify_grand_product", spy("roots", o_gkr.verify_grand_product, 1))
    monkeypatch.setattr(o_kzg, "batch_verify", spy("opening", o_kzg.batch_verify, 5))
    with lcr.installed(lbr.custom_values(case)):
        lbr.verify(pp, [lbr.spec_of(d) for d in descs], n, OT(bytes.fromhex(GOLDEN[case]["proof"])))
    monkeypatch.undo()
    return at


@pytest.mark.parametrize("case", ["two_ranges", "mixed_g"])
def test_a_flipped_byte_in_each_section_is_invalid_snark(hl, vp, pp, monkeypatch, case):
    n = lbr.CASES[case][0]
    proof = bytes.fromhex(GOLDEN[case]["proof"])
    at = _sections(pp, case, monkeypatch)
    assert 32 < at["surge"] < at["roots"] < at["opening"] < len(proof)
    where = {"commitment": 32 + 3, "surge message": at["surge"] + 3, "root": at["roots"] + 3,
             "evaluation": at["opening"] - 29, "opening": at["opening"] + 3, "last quotient": len(proof) - 7}
    tables = tables_of(hl, case)
    for name, pos in where.items():
        bad = bytearray(proof)
        bad[pos] ^= 4
        with pytest.raises(hl.InvalidSnark):
            hl.lasso_verify_batch(vp, tables, n, hl.Keccak256Transcript.from_proof(bytes(bad)))
            pytest.fail("a flipped byte in the %s section verified" % name)


def test_swapped_missing_and_trailing_are_invalid_snark(hl, vp):
    case = "two_ranges"
    n = lbr.CASES[case][0]
    proof = bytes.fromhex(GOLDEN[case]["proof"])
    tables = tables_of(hl, case)
    hl.lasso_verify_batch(vp, tables, n, hl.Keccak256Transcript.from_proof(proof))
    with pytest.raises(hl.InvalidSnark):
        hl.lasso_verify_batch(vp, tables[::-1], n, hl.Keccak256Transcript.from_proof(proof))
    for one in tables:
        with pytest.raises(hl.InvalidSnark):
            hl.lasso_verify_batch(vp, [one], n, hl.Keccak256Transcript.from_proof(proof))
    with pytest.raises(hl.InvalidSnark, match="trailing bytes"):
        hl.lasso_verify_batch(vp, tables, n, hl.Keccak256Transcript.from_proof(proof + b"\0"))
    with pytest.raises(hl.InvalidSnark):  # a proof that ends early
        hl.lasso_verify_batch(vp, tables, n, hl.Keccak256Transcript.from_proof(proof[:-1]))
    # the same tables over AND / XOR: a table is part of the statement
    case = "and_xor_shared"
    proof = bytes.fromhex(GOLDEN[case]["proof"])
    with pytest.raises(hl.InvalidSnark):
        hl.lasso_verify_batch(vp, tables_of(hl, case)[::-1], lbr.CASES[case][0], hl.Keccak256Transcript.from_proof(proof))


def test_single_table_batch_is_not_the_single_proof(hl, vp):
    """K = 1 is not special-cased: its bytes carry K and rho, so neither verifier takes the other's proof"""
    n, descs = lbr.CASES["single"]
    table = lbr.table_of(hl, descs[0])
    proof = bytes.fromhex(GOLDEN["single"]["proof"])
    hl.lasso_verify_batch(vp, [table], n, hl.Keccak256Transcript.from_proof(proof))
    with pytest.raises(hl.Error):
        hl.lasso_verify(vp, table, n, hl.Keccak256Transcript.from_proof(proof))


# ------------------------------------------------------------------ 3. refusals that need no device
def test_argument_refusals(hl, vp):
    from halo2_lasso_amd import _ffi
    lib = _ffi.load()
    assert _ffi.LH_LASSO_BATCH_MAX_TABLES == lbr.MAX_TABLES == 8
    header = open(os.path.join(os.path.dirname(HERE), "include", "lasso_hip.h")).read()
    assert "#define LH_LASSO_BATCH_MAX_TABLES 8\n" in header
    r22 = hl.LassoTable.range(2, 2)
    proof = bytes.fromhex(GOLDEN["two_ranges"]["proof"])
    tr = lambda: hl.Keccak256Transcript.from_proof(proof)
    for tables in ([], [hl.LassoTable.range(1, 2)] * 9):  # K = 0, K = 9
        with pytest.raises(hl.ArgumentError):
            hl.lasso_verify_batch(vp, tables, 4, tr())
        with pytest.raises(hl.ArgumentError):  # (refused before the prover param or the device is touched)
            hl.lasso_prove_batch(None, tables, 4, [[None]] * len(tables), hl.Keccak256Transcript())
    with pytest.raises(hl.ArgumentError):  # one list of columns per table, one column per chunk
        hl.lasso_prove_batch(None, [r22], 4, [], hl.Keccak256Transcript())
    with pytest.raises(hl.ArgumentError):
        hl.lasso_prove_batch(None, [r22], 4, [[None]], hl.Keccak256Transcript())
    # the same through ctypes: the library's own answers
    one = r22.to_c()
    nine = (C.POINTER(_ffi.lh_lasso_table) * 9)(*[C.pointer(one)] * 9)
    t = tr()
    assert lib.lh_lasso_verify_batch(vp.h, nine, 0, 4, t.p) == _ffi.LH_ERR_ARG and b"tables" in lib.lh_last_error()
    assert lib.lh_lasso_verify_batch(vp.h, nine, 9, 4, t.p) == _ffi.LH_ERR_ARG
    assert lib.lh_lasso_verify_batch(vp.h, None, 2, 4, t.p) == _ffi.LH_ERR_ARG  # NULL list
    assert lib.lh_lasso_verify_batch(None, nine, 2, 4, t.p) == _ffi.LH_ERR_ARG  # NULL param
    assert lib.lh_lasso_verify_batch(vp.h, nine, 2, 4, None) == _ffi.LH_ERR_ARG  # NULL transcript
    holed = (C.POINTER(_ffi.lh_lasso_table) * 2)(C.pointer(one), None)
    assert lib.lh_lasso_verify_batch(vp.h, holed, 2, 4, t.p) == _ffi.LH_ERR_ARG  # a NULL table
    assert lib.lh_lasso_verify_batch(vp.h, nine, 2, 0, t.p) == _ffi.LH_ERR_ARG  # no variable
    assert t.remaining() == len(proof), "refused before a byte is read"
    # the prover's entry, as far as it gets without a device: NULL ctx, and never a crash on NULL lists
    assert lib.lh_lasso_prove_batch(None, None, nine, 2, 4, None, t.p) == _ffi.LH_ERR_ARG
    # the sum of the memories: less_than(4, 4) has 7, range(2, 2) has 2
    with pytest.raises(hl.ArgumentError, match="memories"):
        hl.lasso_verify_batch(vp, [hl.LassoTable.less_than(4, 4), r22], 4, tr())
    with pytest.raises(hl.ArgumentError):  # a table lasso_check_table refuses: an odd chunk size under AND
        hl.lasso_verify_batch(vp, [r22, hl.LassoTable.bitwise(hl.SUBTABLE_AND, 2, 3)], 4, tr())
    with pytest.raises(hl.ArgumentError, match="unknown subtable"):
        hl.lasso_verify_batch(vp, [r22, hl.LassoTable(1, 2, [(0, 0xFF)], [(1, [0])])], 4, tr())
    # max(n, max l) above the param: range(1, 7) against the 6-variable param
    with pytest.raises(hl.InvalidPcsParam):
        hl.lasso_verify_batch(vp, [r22, hl.LassoTable.range(1, 7)], 4, tr())
