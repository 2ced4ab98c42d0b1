"""CPU: Spark (lh_spark_commit / lh_spark_open / lh_spark_verify) - the specification (tests/spark_ref.py) against itself,
against two independent statements of the value and against its golden commitments and proofs (tests/golden/spark.json,
tests/golden/make_spark.py); the host verifier on those proofs, on damaged ones and on a cheating prover's; the refusals
that need no device; the exported symbols."""
import ctypes as C
import json
import os
import re

import pytest

import logup_gkr_ref as lgr
import spark_ref as spr
from oracle.pyref import gkr as o_gkr, kzg as o_kzg, sum_check as o_sc
from oracle.pyref.field import R_MOD as P
from oracle.pyref.transcript import Keccak256Transcript as OT

HERE = os.path.dirname(os.path.abspath(__file__))
FILE = json.load(open(os.path.join(HERE, "golden", "spark.json")))
GOLDEN, FORGED = FILE["cases"], FILE["forgeries"]
SS = [int(x, 16) for x in json.load(open(os.path.join(HERE, "golden", "lasso_tables.json")))["srs"]["ss"]]
CASES = list(spr.CASES)
ints = lambda xs: [int(x, 16) for x in xs]


@pytest.fixture(scope="module")
def vp(hl):
    return hl.MultilinearKzgVerifierParams.setup(SS)


@pytest.fixture(scope="module")
def vp_mid(hl):
    return hl.MultilinearKzgVerifierParams.setup(lgr.mid_ss())


@pytest.fixture(scope="module")
def pp():
    return o_kzg.setup(SS)


def opening(case, k=0):
    """-> (commitment, point, value, proof) of a golden opening"""
    g = GOLDEN[case]
    o = g["openings"][k]
    return bytes.fromhex(g["commitment"]), ints(o["point"]), int(o["value"], 16), bytes.fromhex(o["proof"])


def verify(hl, vp, case, k=0, **over):
    n, l, c = spr.CASES[case]
    blob, point, value, proof = opening(case, k)
    a = dict(n=n, l=l, c=c, commitment=blob, point=point, value=value, proof=proof)
    a.update(over)
    hl.spark_verify(vp, a["n"], a["l"], a["c"], a["commitment"], a["point"], a["value"], a["proof"])


# ------------------------------------------------------------------ 1. the specification
def test_the_cases_are_the_named_ones():
    assert set(GOLDEN) == set(spr.CASES) and len(spr.CASES) == 13 and set(FORGED) == set(spr.FORGERIES) == {"bad_e"}
    assert spr.SMALL == [c for c in CASES if c not in ("mid", "wide")] and len(SS) == 6
    for case, (n, l, c) in spr.CASES.items():
        g = GOLDEN[case]
        dims, val = spr.case_entries(case)
        assert (g["n"], g["l"], g["c"]) == (n, l, c) and len(dims) == c and len(val) == 1 << n
        assert all(len(d) == 1 << n and max(d) < 1 << l for d in dims)
        assert len(g["openings"]) == (2 if case == "two_points" else 1)
        assert [ints(o["point"]) for o in g["openings"]] == spr.case_points(case)
    w = lambda case: spr.o_lasso.witness(spr._Spec(*spr.CASES[case][2:0:-1]), spr.case_entries(case)[0])
    mask = lambda case: int.from_bytes(bytes.fromhex(GOLDEN[case]["commitment"])[:32], "big")
    # one_index: every access hits cell 5 - read_ts counts up, one final counter holds them all
    wt = w("one_index")
    assert wt["read_ts"] == [list(range(16))] * 2 and wt["final_cts"] == [[0] * 5 + [16, 0, 0]] * 2
    # distinct: no index twice in a column - read_ts is the zero column and commits to the identity (polys 3 and 4)
    assert not any(any(col) for col in w("distinct")["read_ts"]) and mask("distinct") == 0b11000
    # zero_val: val commits to the identity, the value is 0
    assert mask("zero_val") & 1 and int(GOLDEN["zero_val"]["openings"][0]["value"], 16) == 0
    # duplicates: every index tuple twice
    dims, _ = spr.case_entries("duplicates")
    tuples = list(zip(*dims))
    assert tuples[:4] == tuples[4:]
    # boolean_point: the point is the index tuple of entry 3; the value is the sum of the entries stored there
    dims, val = spr.case_entries("boolean_point")
    at = [k for k in range(16) if all(dims[j][k] == dims[j][3] for j in range(2))]
    assert int(GOLDEN["boolean_point"]["openings"][0]["value"], 16) == sum(val[k] for k in at) % P
    assert set(spr.case_points("boolean_point")[0]) <= {0, 1}
    # big_dims: most cells are never touched
    assert all(sum(1 for x in col if x) <= 4 for col in w("big_dims")["final_cts"])
    # two_points: one commitment, two different points and proofs
    o = GOLDEN["two_points"]["openings"]
    assert o[0]["point"] != o[1]["point"] and o[0]["proof"] != o[1]["proof"]
    assert FILE["bad_value"]["case"] == "matrix"
    assert int(FILE["bad_value"]["value"], 16) == (int(GOLDEN["matrix"]["openings"][0]["value"], 16) + 1) % P


@pytest.mark.parametrize("case", spr.SMALL)
def test_reference_reproduces_the_golden_and_the_value_is_the_defining_sum(pp, case):
    n, l, c = spr.CASES[case]
    dims, val = spr.case_entries(case)
    cm = spr.commit(pp, dims, val, l)
    assert cm.blob.hex() == GOLDEN[case]["commitment"], "the golden commitment is not what the specification produces now"
    for k, point in enumerate(spr.case_points(case)):
        t = OT()
        v = spr.open_(pp, cm, point, t)
        proof = t.into_proof()
        assert proof.hex() == GOLDEN[case]["openings"][k]["proof"] and "%x" % v == GOLDEN[case]["openings"][k]["value"]
        spr.verify(pp, n, l, c, cm.blob, point, v, OT(proof))
        assert v == spr.sparse_eval(dims, val, l, point) == spr.dense_eval(dims, val, l, point)


def test_reference_reproduces_and_refuses_the_forgery(pp):
    n, l, c, dims, val, point, forge = spr.forgery("bad_e")
    g = FORGED["bad_e"]
    assert (g["n"], g["l"], g["c"], g["dims"], g["val"], ints(g["point"])) == (n, l, c, dims, val, point)
    cm = spr.commit(pp, dims, val, l)
    t = OT()
    v = spr.open_(pp, cm, point, t, forge=forge)
    assert t.into_proof().hex() == g["proof"] and "%x" % v == g["value"] and cm.blob.hex() == g["commitment"]
    assert v != spr.sparse_eval(dims, val, l, point), "the forged memory changes the claimed value"
    with pytest.raises(spr.SparkError, match=spr.FORGERIES["bad_e"]):
        spr.verify(pp, n, l, c, cm.blob, point, v, OT(bytes.fromhex(g["proof"])))
    with pytest.raises(spr.SparkError, match="index out of range"):
        spr.commit(pp, [[0, 2, 1, 0], dims[1]], val, l)


# ------------------------------------------------------------------ 2. the host verifier
@pytest.mark.parametrize("case", CASES)
def test_host_verifier_accepts_golden(hl, vp, vp_mid, case):
    for k in range(len(GOLDEN[case]["openings"])):
        verify(hl, vp if case in spr.SMALL else vp_mid, case, k)


def test_host_verifier_refuses_the_forgery_and_a_wrong_value(hl, vp):
    g = FORGED["bad_e"]
    with pytest.raises(hl.InvalidSnark, match=spr.FORGERIES["bad_e"]):
        hl.spark_verify(vp, g["n"], g["l"], g["c"], bytes.fromhex(g["commitment"]), ints(g["point"]), int(g["value"], 16),
                        bytes.fromhex(g["proof"]))
    with pytest.raises(hl.InvalidSnark, match="another value"):
        verify(hl, vp, FILE["bad_value"]["case"], value=int(FILE["bad_value"]["value"], 16))
    with pytest.raises(hl.InvalidSnark, match="another value"):
        verify(hl, vp, "zero_val", value=1)


def _sections(pp, case, monkeypatch):
    """where the sections of a golden proof begin: the specification's verifier is asked, at the entry of its pieces"""
    at = {}

    def spy(name, fn, tr_arg):
        def wrapped(*a, **k):
            at.setdefault(name, a[tr_arg].pos)
            return fn(*a, **k)
        return wrapped

    monkeypatch.setattr(o_sc, "verify", spy("sum-check", o_sc.verify, 4))
    monkeypatch.setattr(o_gkr, "verify_grand_product", spy("grand product", o_gkr.verify_grand_product, 1))
    monkeypatch.setattr(o_kzg, "batch_verify", spy("opening", o_kzg.batch_verify, 5))
    n, l, c = spr.CASES[case]
    blob, point, value, proof = opening(case)
    spr.verify(pp, n, l, c, blob, point, value, OT(proof))
    monkeypatch.undo()
    return at


@pytest.mark.parametrize("case", ["matrix", "cube"])
def test_a_flipped_byte_in_each_section_is_invalid_snark(hl, vp, pp, monkeypatch, case):
    n, l, c = spr.CASES[case]
    blob, point, value, proof = opening(case)
    at = _sections(pp, case, monkeypatch)
    # (no E column of these cases is zero: the mask is 0 and c points follow it; then v)
    assert int.from_bytes(proof[:32], "big") == 0 and at["sum-check"] == 32 + 64 * c + 32
    assert at["grand product"] == at["sum-check"] + 32 * n * (c + 2) + 32 * (c + 1)
    assert at["grand product"] < at["opening"] - 32 * 4 * c and at["opening"] < len(proof)
    where = {"E mask": 31, "E commitments": 32 + 3, "last E commitment": 32 + 64 * c - 5, "v": 32 + 64 * c + 30,
             "sum-check": at["sum-check"] + 3, "sum-check's last round": at["grand product"] - 32 * (c + 1) - 5,
             "evaluations at r_z": at["grand product"] - 7, "grand product roots": at["grand product"] + 3,
             "grand product layers": at["opening"] - 32 * 4 * c - 40, "evaluations at r_N": at["opening"] - 32 * 4 * c + 3,
             "evaluations at r_M": at["opening"] - 29, "opening": at["opening"] + 3, "last quotient": len(proof) - 7}
    for name, pos in where.items():
        bad = bytearray(proof)
        bad[pos] ^= 4
        with pytest.raises(hl.InvalidSnark):
            verify(hl, vp, case, proof=bytes(bad))
            pytest.fail("a flipped byte in the %s section verified" % name)
    # the commitment blob: its mask, a point of each group
    assert len(blob) == 32 + 64 * (1 + 3 * c)
    for pos in (31, 32 + 3, 32 + 64 + 40, 32 + 64 * (1 + c) + 9, len(blob) - 2):
        bad = bytearray(blob)
        bad[pos] ^= 4
        with pytest.raises(hl.InvalidSnark):
            verify(hl, vp, case, commitment=bytes(bad))
            pytest.fail("a flipped byte at %d of the commitment verified" % pos)


def test_other_points_lengths_and_shapes_are_invalid_snark(hl, vp):
    case = "matrix"
    n, l, c = spr.CASES[case]
    blob, point, value, proof = opening(case)
    verify(hl, vp, case)
    for i in (0, l, 2 * l - 1):  # one coordinate of the point: it is part of the statement
        other = list(point)
        other[i] = (other[i] + 1) % P
        with pytest.raises(hl.InvalidSnark):
            verify(hl, vp, case, point=other)
    # two_points: each proof is about its own point and value
    b2, p0, v0, pr0 = opening("two_points", 0)
    _, p1, v1, pr1 = opening("two_points", 1)
    hl.spark_verify(vp, 5, 3, 2, b2, p1, v1, pr1)
    with pytest.raises(hl.InvalidSnark):
        hl.spark_verify(vp, 5, 3, 2, b2, p0, v0, pr1)
    with pytest.raises(hl.InvalidSnark):
        hl.spark_verify(vp, 5, 3, 2, b2, p1, v1, pr0)
    with pytest.raises(hl.InvalidSnark):  # another polynomial's commitment of the same shape
        verify(hl, vp, case, commitment=b2)
    with pytest.raises(hl.InvalidSnark, match="trailing bytes"):
        verify(hl, vp, case, proof=proof + b"\0")
    for cut in (proof[:-1], proof[:700], proof[:40], b""):  # a proof that ends early
        with pytest.raises(hl.InvalidSnark):
            verify(hl, vp, case, proof=cut)
    # a malformed commitment: too short, too long, a mask out of range, a mask that wants fewer points than follow
    for bad in (blob[:-1], blob + b"\0", blob[:32], b"\0" * 31 + b"\x80" + blob[32:], b"\0" * 31 + b"\x01" + blob[32:], b"\1"):
        with pytest.raises(hl.InvalidSnark, match="malformed commitment"):
            verify(hl, vp, case, commitment=bad)
    for other in (dict(n=n - 1), dict(n=n + 1), dict(l=l - 1, point=point[:4]), dict(l=l + 1, point=point + [1, 2]),
                  dict(c=1, point=point[:3]), dict(c=3, point=point + point[:3])):
        with pytest.raises(hl.InvalidSnark):  # another shape
            verify(hl, vp, case, **other)


# ------------------------------------------------------------------ 3. refusals that need no device, the exported symbols
def test_argument_refusals_and_symbols(hl, vp):
    from halo2_lasso_amd import _ffi
    lib = _ffi.load()
    assert (_ffi.LH_SPARK_MAX_DIMS, _ffi.LH_SPARK_MAX_DIM_VARS) == (spr.MAX_DIMS, spr.MAX_DIM_VARS) == (3, 24)
    header = open(os.path.join(os.path.dirname(HERE), "include", "lasso_hip.h")).read()
    assert "#define LH_SPARK_MAX_DIMS 3\n" in header and "#define LH_SPARK_MAX_DIM_VARS 24\n" in header
    for sym in ("lh_spark_commit", "lh_spark_commitment", "lh_spark_open", "lh_spark_verify", "lh_debug_spark_e"):
        assert hasattr(lib, sym) and sym in _ffi.SIGNATURES and re.search(r"lh_status %s\(" % sym, header), sym
    assert hasattr(lib, "lh_spark_free") and re.search(r"void lh_spark_free\(", header)
    rust = open(os.path.join(os.path.dirname(HERE), "bindings", "rust", "src", "sys.rs")).read()
    for sym in ("lh_spark_commit", "lh_spark_commitment", "lh_spark_open", "lh_spark_free", "lh_spark_verify", "lh_debug_spark_e"):
        assert re.search(r"pub fn %s\(" % sym, rust), sym
    case = "matrix"
    n, l, c = spr.CASES[case]
    blob, point, value, proof = opening(case)
    for bad in (dict(n=0), dict(n=31), dict(l=0, point=[]), dict(l=25, point=point * 9), dict(c=0, point=[]),
                dict(c=4, point=point * 2), dict(point=point[:-1]), dict(point=point + [0]), dict(commitment=None),
                dict(proof=None), dict(value=None)):
        with pytest.raises(hl.ArgumentError):
            verify(hl, vp, case, **bad)
    # max(n, l) above the param: seven variables against the 6-variable param, either way
    with pytest.raises(hl.InvalidPcsParam):
        verify(hl, vp, case, n=7)
    with pytest.raises(hl.InvalidPcsParam):
        verify(hl, vp, case, l=7, point=(point * 3)[:14])
    # the same through ctypes: the library's own answers
    tr = lambda: hl.Keccak256Transcript.from_proof(proof)
    cm = (C.c_uint8 * len(blob)).from_buffer_copy(blob)
    pt, val = hl._fr_array(point), hl._fr_array([value])
    t = tr()
    assert lib.lh_spark_verify(vp.h, n, l, c, cm, len(blob), pt, val, tr().p) == _ffi.LH_OK
    assert lib.lh_spark_verify(None, n, l, c, cm, len(blob), pt, val, t.p) == _ffi.LH_ERR_ARG  # NULL param
    assert lib.lh_spark_verify(vp.h, n, l, c, None, len(blob), pt, val, t.p) == _ffi.LH_ERR_ARG  # NULL commitment
    assert lib.lh_spark_verify(vp.h, n, l, c, cm, len(blob), None, val, t.p) == _ffi.LH_ERR_ARG  # NULL point
    assert lib.lh_spark_verify(vp.h, n, l, c, cm, len(blob), pt, None, t.p) == _ffi.LH_ERR_ARG  # NULL value
    assert lib.lh_spark_verify(vp.h, n, l, c, cm, len(blob), pt, val, None) == _ffi.LH_ERR_ARG  # NULL transcript
    for bn, bl, bc, word in ((0, l, c, b"num_vars"), (31, l, c, b"num_vars"), (n, 0, c, b"dim_vars"), (n, 25, c, b"dim_vars"),
                             (n, l, 0, b"num_dims"), (n, l, 4, b"num_dims")):
        assert lib.lh_spark_verify(vp.h, bn, bl, bc, cm, len(blob), pt, val, t.p) == _ffi.LH_ERR_ARG, (bn, bl, bc)
        assert word in lib.lh_last_error()
    assert lib.lh_spark_verify(vp.h, 7, l, c, cm, len(blob), pt, val, t.p) == _ffi.LH_ERR_INVALID_PCS_PARAM
    assert lib.lh_spark_verify(vp.h, n, l, c, cm, len(blob) - 1, pt, val, t.p) == _ffi.LH_ERR_INVALID_SNARK
    assert b"malformed commitment" in lib.lh_last_error()
    assert t.remaining() == len(proof), "refused before a byte is read"
    # the prover's entries as far as they get without a device: the shape, then the NULL ctx; never a crash on NULL lists
    h = C.c_void_p()
    assert lib.lh_spark_commit(None, None, n, l, c, None, None, C.byref(h)) == _ffi.LH_ERR_ARG and not h.value
    assert lib.lh_spark_commit(None, None, n, l, 4, None, None, C.byref(h)) == _ffi.LH_ERR_ARG
    assert b"num_dims" in lib.lh_last_error()
    assert lib.lh_spark_commit(None, None, n, 25, c, None, None, C.byref(h)) == _ffi.LH_ERR_ARG
    assert b"dim_vars" in lib.lh_last_error()
    size = C.c_size_t(0)
    assert lib.lh_spark_commitment(None, None, C.byref(size)) == _ffi.LH_ERR_ARG
    assert lib.lh_spark_open(None, None, None, pt, val, t.p) == _ffi.LH_ERR_ARG
    assert lib.lh_debug_spark_e(None, n, l, c, None, None, pt, None, val) == _ffi.LH_ERR_ARG
    lib.lh_spark_free(None, None)  # (nothing to do, nothing to crash on)
    with pytest.raises(hl.ArgumentError):  # refused before the ctx or the device is touched
        hl.spark_commit(None, None, [1, 2, 3, 4], 5, l, num_vars=n)
    with pytest.raises(hl.ArgumentError):
        hl.spark_commit(None, None, [1, 2], 5, 25, num_vars=n)
    with pytest.raises(hl.ArgumentError):
        hl.spark_commit(None, None, [1, None], 5, l, num_vars=n)
    with pytest.raises(hl.ArgumentError):  # raw pointers without num_vars
        hl.spark_commit(None, None, [1, 2], 5, l)
