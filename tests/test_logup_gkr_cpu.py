"""CPU: the LogUp-GKR lookup argument (lh_logup_gkr_prove / lh_logup_gkr_verify) and the host verifier of the fractional
sum-check (lh_gkr_fractional_verify) - the specification (tests/logup_gkr_ref.py) against itself and against its golden
proofs (tests/golden/logup_gkr.json, tests/golden/make_logup_gkr.py), the host verifier on those proofs, on damaged ones
and on a cheating prover's, lh_gkr_fractional_verify against oracle/pyref/gkr.py, and the refusals that need no device."""
import ctypes as C
import json
import os
import random

import pytest

import logup_gkr_ref as lgr
from oracle.pyref import gkr as o_gkr, kzg as o_kzg, sum_check as o_sc
from oracle.pyref.field import R_MOD as P
from oracle.pyref.transcript import Keccak256Transcript as OT

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "logup_gkr.json")))["cases"]
SS = [int(x, 16) for x in json.load(open(os.path.join(HERE, "golden", "lasso_tables.json")))["srs"]["ss"]]
CASES = list(lgr.CASES)


@pytest.fixture(scope="module")
def vp(hl):
    return hl.MultilinearKzgVerifierParams.setup(SS)


@pytest.fixture(scope="module")
def vp_mid(hl):
    return hl.MultilinearKzgVerifierParams.setup(lgr.mid_ss())


@pytest.fixture(scope="module")
def pp():
    return o_kzg.setup(SS)


def statement(hl, case, tables=None):
    return [hl.LogupLookup(None, t) for t in (tables or lgr.case_tables(case))]


def proof_of(case):
    return bytes.fromhex(GOLDEN[case]["proof"])


# ------------------------------------------------------------------ 1. the specification
def test_the_cases_are_the_named_ones():
    assert set(GOLDEN) == set(lgr.CASES) and len(lgr.CASES) == 9
    assert lgr.SMALL == [c for c in CASES if c != "mid"] and len(SS) == 6 and len(lgr.mid_ss()) == 14
    for case, (n, l, widths) in lgr.CASES.items():
        g = GOLDEN[case]
        assert (g["n"], g["l"], g["widths"]) == (n, l, widths) and g["rows"] == lgr.case_rows(case)
    mult = lambda case: lgr.multiplicities(*[cols[0] for cols in lgr.case_lookups(case)[0]])
    # dup: rows 2, 5, 7 hold one value and every count of it is on row 7
    t = lgr.case_tables("dup")[0][0]
    m = mult("dup")
    assert t[2] == t[5] == t[7] and m[2] == m[5] == 0 and m[7] >= 5 and sum(m) == 16
    # zeros: everything is zero, every count on the last row
    assert not any(lgr.case_tables("zeros")[0][0]) and mult("zeros") == [0] * 7 + [16]
    # one_row: a tuple of two, one non-zero count
    beta = 12345
    (f, t), = lgr.case_lookups("one_row")
    assert lgr.multiplicities(lgr.compress(f, beta), lgr.compress(t, beta)) == [0, 0, 0, 16, 0, 0, 0, 0]
    # collide: two different values whose Montgomery forms share their low 64 bits, both looked up
    t = lgr.case_tables("collide")[0][0]
    mont = lambda v: v * (1 << 256) % P
    assert t[1] != t[6] and mont(t[1]) % (1 << 64) == mont(t[6]) % (1 << 64)
    m = mult("collide")
    assert m[1] >= 2 and m[6] >= 2


@pytest.mark.parametrize("case", lgr.SMALL)
def test_reference_proves_verifies_and_matches_golden(pp, case):
    lookups = lgr.case_lookups(case)
    t = OT()
    lgr.prove(pp, lookups, t)
    proof = t.into_proof()
    lgr.verify(pp, [tb for _, tb in lookups], lgr.CASES[case][0], OT(proof))
    assert proof.hex() == GOLDEN[case]["proof"], "the golden bytes are not what the specification produces now"


# ------------------------------------------------------------------ 2. the host verifier
@pytest.mark.parametrize("case", CASES)
def test_host_verifier_accepts_golden(hl, vp, vp_mid, case):
    tr = hl.Keccak256Transcript.from_proof(proof_of(case))
    hl.logup_gkr_verify(vp if case in lgr.SMALL else vp_mid, statement(hl, case), lgr.CASES[case][0], tr)
    assert tr.remaining() == 0


def _sections(pp, case, monkeypatch):
    """where the sections of a golden proof begin: the specification's verifier is asked, at the entry of its pieces"""
    at = {}

    def spy(name, fn, tr_arg):
        def wrapped(*a, **k):
            at.setdefault(name, a[tr_arg].pos)
            return fn(*a, **k)
        return wrapped

    monkeypatch.setattr(lgr, "verify_fractional_sum_check", spy("roots", lgr.verify_fractional_sum_check, 2))
    monkeypatch.setattr(o_sc, "verify", spy("round", o_sc.verify, 4))
    monkeypatch.setattr(o_kzg, "batch_verify", spy("opening", o_kzg.batch_verify, 5))
    lgr.verify(pp, lgr.case_tables(case), lgr.CASES[case][0], OT(proof_of(case)))
    monkeypatch.undo()
    return at


@pytest.mark.parametrize("case", ["small_table", "square"])
def test_a_flipped_byte_in_each_section_is_invalid_snark(hl, vp, pp, monkeypatch, case):
    n, l, widths = lgr.CASES[case]
    proof = proof_of(case)
    at = _sections(pp, case, monkeypatch)
    m_block = 32 + 64 * sum(widths)  # (no input column of these cases is zero: the mask is 0)
    assert int.from_bytes(proof[:32], "little") == 0 and m_block < at["roots"] < at["round"] < at["opening"] < len(proof)
    where = {"commitments": 32 + 3, "m block": m_block + 32 + 3, "roots": at["roots"] + 3, "round message": at["round"] + 3,
             "evaluations": at["opening"] - 29, "opening": at["opening"] + 3, "last quotient": len(proof) - 7}
    lookups = statement(hl, case)
    for name, pos in where.items():
        bad = bytearray(proof)
        bad[pos] ^= 4
        with pytest.raises(hl.InvalidSnark):
            hl.logup_gkr_verify(vp, lookups, n, hl.Keccak256Transcript.from_proof(bytes(bad)))
            pytest.fail("a flipped byte in the %s section verified" % name)


def test_changed_table_swapped_trailing_and_truncated_are_invalid_snark(hl, vp):
    case = "small_table"
    n = lgr.CASES[case][0]
    proof = proof_of(case)
    tr = lambda p=proof: hl.Keccak256Transcript.from_proof(p)
    tables = lgr.case_tables(case)
    hl.logup_gkr_verify(vp, statement(hl, case), n, tr())
    changed = [[list(col) for col in t] for t in tables]  # one entry of the table: it is part of the statement
    changed[0][1][5] = (changed[0][1][5] + 1) % P
    with pytest.raises(hl.InvalidSnark):
        hl.logup_gkr_verify(vp, statement(hl, case, changed), n, tr())
    with pytest.raises(hl.InvalidSnark):  # swapped lookups (widths 3 and 1: the header differs)
        hl.logup_gkr_verify(vp, statement(hl, case, tables[::-1]), n, tr())
    sq = lgr.case_tables("square")  # (widths 1 and 2; swapped tables of one width: the same header, other tables)
    with pytest.raises(hl.InvalidSnark):
        hl.logup_gkr_verify(vp, statement(hl, "square", [sq[0], [sq[1][1], sq[1][0]]]), 6, tr(proof_of("square")))
    with pytest.raises(hl.InvalidSnark, match="trailing bytes"):
        hl.logup_gkr_verify(vp, statement(hl, case), n, tr(proof + b"\0"))
    with pytest.raises(hl.InvalidSnark):  # a proof that ends early
        hl.logup_gkr_verify(vp, statement(hl, case), n, tr(proof[:-1]))
    with pytest.raises(hl.InvalidSnark):
        hl.logup_gkr_verify(vp, statement(hl, case), n, tr(proof[:700]))
    with pytest.raises(hl.InvalidSnark):  # another num_vars
        hl.logup_gkr_verify(vp, statement(hl, case), n - 1, tr())


def test_a_cheating_prover_is_rejected_at_the_roots(hl, vp, pp):
    """an input that is in no table row, and multiplicities made up for it: every sum-check and the opening are honest
    about the forged columns, so the only thing left to fail is the LogUp identity on the roots"""
    n, l, widths = lgr.CASES["dup"]
    (f, t), = lgr.case_lookups("dup")
    f = [list(f[0])]
    f[0][9] = (max(t[0]) + 1) % P if (max(t[0]) + 1) % P not in t[0] else 1
    assert f[0][9] not in t[0]
    with pytest.raises(lgr.LogupError, match="Invalid lookup input"):
        lgr.prove(pp, [(f, t)], OT())

    def forge(k, cf, ct):  # the missing input is counted on row 0
        m = [0] * len(ct)
        for v in cf:
            m[ct.index(v) if v in ct else 0] += 1
        return m

    tr = OT()
    lgr.prove(pp, [(f, t)], tr, forge=forge)
    proof = tr.into_proof()
    with pytest.raises(lgr.LogupError, match="do not sum to zero"):
        lgr.verify(pp, [t], n, OT(proof))
    with pytest.raises(hl.InvalidSnark, match="do not sum to zero"):
        hl.logup_gkr_verify(vp, [hl.LogupLookup(None, t)], n, hl.Keccak256Transcript.from_proof(proof))


# ------------------------------------------------------------------ 3. lh_gkr_fractional_verify against the oracle
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("num_vars", [1, 2, 3, 4, 5])
def test_fractional_verify_matches_the_oracle(hl, B, num_vars):
    rng = random.Random(1000 * B + num_vars)
    ps = [[rng.randrange(P) for _ in range(1 << num_vars)] for _ in range(B)]
    qs = [[rng.randrange(1, P) for _ in range(1 << num_vars)] for _ in range(B)]
    none = [None] * B
    t = OT()
    want = o_gkr.prove_fractional_sum_check(none, none, ps, qs, t)
    proof = t.into_proof()
    assert o_gkr.verify_fractional_sum_check(num_vars, none, none, OT(proof)) == want
    roots = OT(proof).read_field_elements(2 * B)
    tr = hl.Keccak256Transcript.from_proof(proof)
    p_0s, q_0s, p_xs, q_xs, x = hl.verify_fractional_sum_check(num_vars, none, none, tr)
    assert (p_xs, q_xs, x) == tuple(want) and p_0s + q_0s == roots and tr.remaining() == 0
    # roots given: hashed, not written; the second fraction's q stays a written root when there is one
    given_p = roots[:B]
    given_q = [v if b != 1 else None for b, v in enumerate(roots[B:])]
    t = OT()
    want_given = o_gkr.prove_fractional_sum_check(given_p, given_q, ps, qs, t)
    proof_given = t.into_proof()
    assert o_gkr.verify_fractional_sum_check(num_vars, given_p, given_q, OT(proof_given)) == want_given
    assert len(proof_given) == len(proof) - 32 * (2 * B - given_q.count(None))
    tr = hl.Keccak256Transcript.from_proof(proof_given)
    got = hl.verify_fractional_sum_check(num_vars, given_p, given_q, tr)
    assert got == (roots[:B], roots[B:]) + tuple(want_given) and tr.remaining() == 0
    # damage: a root that is read, a claim that is given, an evaluation
    for bad_proof, claims in ((flip(proof, 3), (none, none)), (flip(proof, len(proof) - 32 * 4 * B + 3), (none, none)),
                              (proof_given, ([(given_p[0] + 1) % P] + given_p[1:], given_q))):
        with pytest.raises(hl.InvalidSumcheck):
            hl.verify_fractional_sum_check(num_vars, claims[0], claims[1], hl.Keccak256Transcript.from_proof(bad_proof))
    with pytest.raises(hl.Error):  # a proof that ends early: the transcript's own error
        hl.verify_fractional_sum_check(num_vars, none, none, hl.Keccak256Transcript.from_proof(proof[:-32]))


def flip(proof, pos):
    bad = bytearray(proof)
    bad[pos] ^= 4
    return bytes(bad)


def test_fractional_verify_refusals(hl):
    tr = hl.Keccak256Transcript.from_proof(bytes(64))
    for B, num_vars in ((0, 3), (1, 0), (17, 3)):
        with pytest.raises(hl.ArgumentError):
            hl.verify_fractional_sum_check(num_vars, [None] * B, [None] * B, tr)
    with pytest.raises(hl.ArgumentError):
        hl.verify_fractional_sum_check(3, [None], [None, None], tr)
    from halo2_lasso_amd import _ffi
    assert _ffi.load().lh_gkr_fractional_verify(1, 3, None, None, None, None, None, None, None, None) == _ffi.LH_ERR_ARG
    assert tr.remaining() == 64, "refused before a byte is read"


# ------------------------------------------------------------------ 4. refusals that need no device
def test_argument_refusals(hl, vp):
    from halo2_lasso_amd import _ffi
    lib = _ffi.load()
    assert (_ffi.LH_LOGUP_MAX_LOOKUPS, _ffi.LH_LOGUP_MAX_WIDTH, _ffi.LH_LOGUP_MAX_TABLE_VARS) == \
        (lgr.MAX_LOOKUPS, lgr.MAX_WIDTH, lgr.MAX_TABLE_VARS) == (8, 8, 24)
    header = open(os.path.join(os.path.dirname(HERE), "include", "lasso_hip.h")).read()
    for line in ("#define LH_LOGUP_MAX_LOOKUPS 8\n", "#define LH_LOGUP_MAX_WIDTH 8\n", "#define LH_LOGUP_MAX_TABLE_VARS 24\n"):
        assert line in header
    proof = proof_of("dup")
    tr = lambda: hl.Keccak256Transcript.from_proof(proof)
    col = lgr.case_tables("dup")[0][0]
    one = hl.LogupLookup(None, [col])
    hl.logup_gkr_verify(vp, [one], 4, tr())
    bad = {"no lookup": [], "nine lookups": [one] * 9, "width 0": [hl.LogupLookup(None, [])],
           "width 9": [hl.LogupLookup(None, [col] * 9)], "ragged": [hl.LogupLookup(None, [col, col[:4]])],
           "one row": [hl.LogupLookup(None, [[5]])], "not a power of two": [hl.LogupLookup(None, [col[:6]])],
           "two table sizes": [one, hl.LogupLookup(None, [col[:4]])], "64 columns": [hl.LogupLookup(None, [col] * 8)] * 8}
    for name, lookups in bad.items():
        with pytest.raises(hl.ArgumentError):
            hl.logup_gkr_verify(vp, lookups, 4, tr())
            pytest.fail(name)
        with pytest.raises(hl.ArgumentError):  # (refused before the prover param or the device is touched)
            hl.logup_gkr_prove(None, [hl.LogupLookup([None] * lk.width, lk.table) for lk in lookups], hl.Keccak256Transcript(), 4)
            pytest.fail(name)
    for n in (0, 31):
        with pytest.raises(hl.ArgumentError):
            hl.logup_gkr_verify(vp, [one], n, tr())
        with pytest.raises(hl.ArgumentError):
            hl.logup_gkr_prove(None, [hl.LogupLookup([None], [col])], hl.Keccak256Transcript(), n)
    with pytest.raises(hl.ArgumentError):  # the inputs of a prover: one per table column
        hl.logup_gkr_prove(None, [hl.LogupLookup([None, None], [col])], hl.Keccak256Transcript(), 4)
    with pytest.raises(hl.ArgumentError):
        hl.logup_gkr_prove(None, [one], hl.Keccak256Transcript(), 4)
    # max(n, l) above the param: seven variables against the 6-variable param, either way
    with pytest.raises(hl.InvalidPcsParam):
        hl.logup_gkr_verify(vp, [one], 7, tr())
    with pytest.raises(hl.InvalidPcsParam):
        hl.logup_gkr_verify(vp, [hl.LogupLookup(None, [col * 16])], 4, tr())
    # the same through ctypes: the library's own answers
    cols = hl._fr_array(col)
    tab = (C.POINTER(_ffi.lh_fr) * 9)(*[C.cast(cols, C.POINTER(_ffi.lh_fr))] * 9)

    def arr(count, width=1, table=tab):
        a = (_ffi.lh_logup_lookup * max(count, 1))()
        for k in range(count):
            a[k].width, a[k].table = width, table
        return a

    t = tr()
    good = arr(1)
    assert lib.lh_logup_gkr_verify(vp.h, good, 1, 4, 3, hl.Keccak256Transcript.from_proof(proof).p) == _ffi.LH_OK
    assert lib.lh_logup_gkr_verify(vp.h, good, 0, 4, 3, t.p) == _ffi.LH_ERR_ARG and b"lookups" in lib.lh_last_error()
    assert lib.lh_logup_gkr_verify(vp.h, arr(9), 9, 4, 3, t.p) == _ffi.LH_ERR_ARG
    assert lib.lh_logup_gkr_verify(vp.h, None, 1, 4, 3, t.p) == _ffi.LH_ERR_ARG  # NULL list
    assert lib.lh_logup_gkr_verify(None, good, 1, 4, 3, t.p) == _ffi.LH_ERR_ARG  # NULL param
    assert lib.lh_logup_gkr_verify(vp.h, good, 1, 4, 3, None) == _ffi.LH_ERR_ARG  # NULL transcript
    assert lib.lh_logup_gkr_verify(vp.h, arr(1, 1, None), 1, 4, 3, t.p) == _ffi.LH_ERR_ARG  # NULL table
    holed = (C.POINTER(_ffi.lh_fr) * 2)(C.cast(cols, C.POINTER(_ffi.lh_fr)), None)
    assert lib.lh_logup_gkr_verify(vp.h, arr(1, 2, holed), 1, 4, 3, t.p) == _ffi.LH_ERR_ARG  # a NULL table column
    assert lib.lh_logup_gkr_verify(vp.h, arr(1, 0), 1, 4, 3, t.p) == _ffi.LH_ERR_ARG and b"width" in lib.lh_last_error()
    assert lib.lh_logup_gkr_verify(vp.h, arr(1, 9), 1, 4, 3, t.p) == _ffi.LH_ERR_ARG
    assert lib.lh_logup_gkr_verify(vp.h, arr(8, 8), 8, 4, 3, t.p) == _ffi.LH_ERR_ARG and b"63" in lib.lh_last_error()
    for n, l in ((0, 3), (31, 3), (4, 0), (4, 25)):
        assert lib.lh_logup_gkr_verify(vp.h, good, 1, n, l, t.p) == _ffi.LH_ERR_ARG, (n, l)
    assert lib.lh_logup_gkr_verify(vp.h, good, 1, 7, 3, t.p) == _ffi.LH_ERR_INVALID_PCS_PARAM
    assert t.remaining() == len(proof), "refused before a byte is read"
    # the prover's entry, as far as it gets without a device: NULL ctx, and never a crash on NULL lists
    assert lib.lh_logup_gkr_prove(None, None, good, 1, 4, 3, t.p) == _ffi.LH_ERR_ARG
    assert lib.lh_logup_gkr_prove(None, None, None, 1, 4, 3, None) == _ffi.LH_ERR_ARG
