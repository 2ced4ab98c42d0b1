"""CPU: the read-write memory-checking argument (lh_memcheck_prove / lh_memcheck_verify) - the specification
(tests/memcheck_ref.py) against itself and against its golden proofs (tests/golden/memcheck.json,
tests/golden/make_memcheck.py), the host verifier on those proofs, on damaged ones and on two cheating provers', and the
refusals that need no device."""
import ctypes as C
import json
import os
import re

import pytest

import logup_gkr_ref as lgr
import memcheck_ref as mcr
from oracle.pyref import gkr as o_gkr, kzg as o_kzg
from oracle.pyref.transcript import Keccak256Transcript as OT

HERE = os.path.dirname(os.path.abspath(__file__))
FILE = json.load(open(os.path.join(HERE, "golden", "memcheck.json")))
GOLDEN, FORGED = FILE["cases"], FILE["forgeries"]
SS = [int(x, 16) for x in json.load(open(os.path.join(HERE, "golden", "lasso_tables.json")))["srs"]["ss"]]
CASES = list(mcr.CASES)


@pytest.fixture(scope="module")
def vp(hl):
    return hl.MultilinearKzgVerifierParams.setup(SS)


@pytest.fixture(scope="module")
def vp_mid(hl):
    return hl.MultilinearKzgVerifierParams.setup(lgr.mid_ss())


@pytest.fixture(scope="module")
def pp():
    return o_kzg.setup(SS)


def proof_of(case):
    return bytes.fromhex(GOLDEN[case]["proof"])


def verify(hl, vp, case, proof=None, **over):
    n, l, _ = mcr.CASES[case]
    a = dict(n=n, l=l, init=mcr.case_init(case))
    a.update(over)
    tr = hl.Keccak256Transcript.from_proof(proof_of(case) if proof is None else proof)
    hl.memcheck_verify(vp, a["n"], a["l"], tr, init=a["init"])
    return tr


# ------------------------------------------------------------------ 1. the specification
def test_the_cases_are_the_named_ones():
    assert set(GOLDEN) == set(mcr.CASES) and len(mcr.CASES) == 10 and set(FORGED) == set(mcr.FORGERIES)
    assert mcr.SMALL == [c for c in CASES if c not in ("mid", "wide")] and len(SS) == 6
    for case, (n, l, has_init) in mcr.CASES.items():
        g = GOLDEN[case]
        assert (g["n"], g["l"], g["init"]) == (n, l, has_init) and (mcr.case_init(case) is not None) == has_init
        addr, rv, wv = mcr.case_trace(case)
        assert len(addr) == len(rv) == len(wv) == 1 << n and max(addr) < 1 << l and max(rv + wv) < 1 << 32
    N = lambda case: 1 << mcr.CASES[case][0]
    wit = lambda case: mcr.witness(*mcr.case_trace(case), mcr.case_init(case) or [0] * (1 << mcr.CASES[case][1]))
    # one_cell: every operation on cell 0, so every difference i - rt[i] is 0
    w = wit("one_cell")
    assert set(mcr.case_trace("one_cell")[0]) == {0} and w["m"] == [N("one_cell")] + [0] * (N("one_cell") - 1)
    assert w["rt"] == list(range(N("one_cell")))
    # distinct: no cell twice - rt is the zero column (an identity commitment), difference i once each
    w = wit("distinct")
    assert len(set(mcr.case_trace("distinct")[0])) == N("distinct") and not any(w["rt"]) and w["m"] == [1] * N("distinct")
    assert int.from_bytes(proof_of("distinct")[:32], "big") == 1 << 3, "the mask names rt, commitment 3, as the identity"
    # loads_only: the memory ends as it began
    assert wit("loads_only")["fv"] == mcr.case_init("loads_only")
    # big_mem: cells nobody touches keep the image and time 0
    w, touched = wit("big_mem"), set(mcr.case_trace("big_mem")[0])
    assert len(touched) < 16
    assert all(w["ft"][a] == 0 and w["fv"][a] == mcr.case_init("big_mem")[a] for a in range(16) if a not in touched)
    # edges: every edge word is stored and read back
    addr, rv, wv = mcr.case_trace("edges")
    assert set(mcr.EDGE_WORDS) <= set(wv) and set(mcr.EDGE_WORDS) <= set(rv) and mcr.EDGE_WORDS[-1] == 0xFFFFFFFF
    # small_mem: many repeats per cell
    assert max(wit("small_mem")["m"][1:]) >= 1 and len(set(mcr.case_trace("small_mem")[0])) <= 8


def test_the_specification_refuses_inconsistent_traces(pp):
    addr, rv, wv = mcr.case_trace("small_mem")
    init = mcr.case_init("small_mem")
    for at in (0, 13, 31):
        bad = list(rv)
        bad[at] ^= 1
        with pytest.raises(mcr.MemcheckError, match="Invalid memory trace"):
            mcr.prove(pp, addr, bad, wv, 3, init, OT())
    with pytest.raises(mcr.MemcheckError, match="Invalid memory trace"):
        mcr.prove(pp, [8] + addr[1:], rv, wv, 3, init, OT())


@pytest.mark.parametrize("case", mcr.SMALL)
def test_reference_proves_verifies_and_matches_golden(pp, case):
    n, l, _ = mcr.CASES[case]
    init = mcr.case_init(case)
    t = OT()
    mcr.prove(pp, *mcr.case_trace(case), l, init, t)
    proof = t.into_proof()
    mcr.verify(pp, n, l, init, OT(proof))
    assert proof.hex() == GOLDEN[case]["proof"], "the golden bytes are not what the specification produces now"


@pytest.mark.parametrize("name", list(mcr.FORGERIES))
def test_reference_reproduces_and_refuses_the_forgeries(pp, name):
    n, l, trace, forge = mcr.forgery(name)
    g = FORGED[name]
    assert (g["n"], g["l"], (g["addr"], g["rv"], g["wv"])) == (n, l, tuple(trace))
    with pytest.raises(mcr.MemcheckError, match="Invalid memory trace"):  # the honest prover has no proof of these traces
        mcr.prove(pp, *trace, l, None, OT())
    t = OT()
    mcr.prove(pp, *trace, l, None, t, forge=forge)
    assert t.into_proof().hex() == g["proof"]
    with pytest.raises(mcr.MemcheckError, match=mcr.FORGERIES[name]):
        mcr.verify(pp, n, l, None, OT(bytes.fromhex(g["proof"])))


# ------------------------------------------------------------------ 2. the host verifier
@pytest.mark.parametrize("case", CASES)
def test_host_verifier_accepts_golden(hl, vp, vp_mid, case):
    assert verify(hl, vp if case in mcr.SMALL else vp_mid, case).remaining() == 0


@pytest.mark.parametrize("name", list(mcr.FORGERIES))
def test_host_verifier_refuses_the_forgeries_where_it_should(hl, vp, name):
    """future_read: every sum-check and the opening are honest about the forged columns and the multisets are equal, so
    the only thing left to fail is the range check on the fractions' roots; stale_read dies at the multiset identity"""
    g = FORGED[name]
    with pytest.raises(hl.InvalidSnark, match=mcr.FORGERIES[name]):
        hl.memcheck_verify(vp, g["n"], g["l"], hl.Keccak256Transcript.from_proof(bytes.fromhex(g["proof"])))


def _sections(pp, case, monkeypatch):
    """where the sections of a golden proof begin: the specification's verifier is asked, at the entry of its pieces"""
    at = {}

    def spy(name, fn, tr_arg):
        def wrapped(*a, **k):
            at.setdefault(name, a[tr_arg].pos)
            return fn(*a, **k)
        return wrapped

    monkeypatch.setattr(o_gkr, "verify_grand_product", spy("grand product", o_gkr.verify_grand_product, 1))
    monkeypatch.setattr(lgr, "verify_fractional_sum_check", spy("fractions", lgr.verify_fractional_sum_check, 2))
    monkeypatch.setattr(o_kzg, "batch_verify", spy("opening", o_kzg.batch_verify, 5))
    n, l, _ = mcr.CASES[case]
    mcr.verify(pp, n, l, mcr.case_init(case), OT(proof_of(case)))
    monkeypatch.undo()
    return at


@pytest.mark.parametrize("case", ["small_mem", "square"])
def test_a_flipped_byte_in_each_section_is_invalid_snark(hl, vp, pp, monkeypatch, case):
    proof = proof_of(case)
    at = _sections(pp, case, monkeypatch)
    # (no column of these cases is zero: the mask is 0 and seven points follow it)
    assert int.from_bytes(proof[:32], "little") == 0 and at["grand product"] == 32 + 64 * mcr.NUM_POLYS
    assert at["grand product"] < at["fractions"] < at["opening"] - 32 * len(mcr.OPENINGS) and at["opening"] < len(proof)
    where = {"commitments": 32 + 3, "last commitment": at["grand product"] - 5, "grand product roots": at["grand product"] + 3,
             "grand product layers": at["fractions"] - 40, "fractions' roots": at["fractions"] + 3,
             "fractions' layers": at["opening"] - 32 * len(mcr.OPENINGS) - 40, "evaluations": at["opening"] - 29,
             "first evaluation": at["opening"] - 32 * len(mcr.OPENINGS) + 3, "opening": at["opening"] + 3,
             "last quotient": len(proof) - 7}
    for name, pos in where.items():
        bad = bytearray(proof)
        bad[pos] ^= 4
        with pytest.raises(hl.InvalidSnark):
            verify(hl, vp, case, bytes(bad))
            pytest.fail("a flipped byte in the %s section verified" % name)


def test_changed_image_trailing_and_truncated_are_invalid_snark(hl, vp):
    case = "small_mem"
    n, l, _ = mcr.CASES[case]
    proof, init = proof_of(case), mcr.case_init(case)
    verify(hl, vp, case)
    for a in (0, 5, 7):  # one word of the image: it is part of the statement
        changed = list(init)
        changed[a] ^= 1 << (4 * a)
        with pytest.raises(hl.InvalidSnark):
            verify(hl, vp, case, init=changed)
    with pytest.raises(hl.InvalidSnark):  # image given vs none: the header differs
        verify(hl, vp, case, init=None)
    with pytest.raises(hl.InvalidSnark):
        verify(hl, vp, "square", init=[0] * 64)
    with pytest.raises(hl.InvalidSnark):  # an all-zero image given for a proof about no image: the same cells, another statement
        verify(hl, vp, "one_var", init=[0, 0])
    with pytest.raises(hl.InvalidSnark, match="trailing bytes"):
        verify(hl, vp, case, proof + b"\0")
    with pytest.raises(hl.InvalidSnark):  # a proof that ends early
        verify(hl, vp, case, proof[:-1])
    with pytest.raises(hl.InvalidSnark):
        verify(hl, vp, case, proof[:700])
    with pytest.raises(hl.InvalidSnark):
        verify(hl, vp, case, b"")
    for other in (dict(n=n - 1), dict(n=n + 1), dict(l=l - 1, init=init[:4]), dict(l=l + 1, init=init * 2)):
        with pytest.raises(hl.InvalidSnark):  # another shape
            verify(hl, vp, case, **other)


# ------------------------------------------------------------------ 3. refusals that need no device
def test_argument_refusals(hl, vp):
    from halo2_lasso_amd import _ffi
    lib = _ffi.load()
    assert _ffi.LH_MEMCHECK_MAX_INIT_VARS == mcr.MAX_INIT_VARS == 24
    header = open(os.path.join(os.path.dirname(HERE), "include", "lasso_hip.h")).read()
    assert "#define LH_MEMCHECK_MAX_INIT_VARS 24\n" in header
    for sym in ("lh_memcheck_prove", "lh_memcheck_verify", "lh_debug_memcheck_witness"):
        assert hasattr(lib, sym) and sym in _ffi.SIGNATURES and re.search(r"lh_status %s\(" % sym, header)
    case = "small_mem"
    n, l, _ = mcr.CASES[case]
    proof, init = proof_of(case), mcr.case_init(case)
    tr = lambda: hl.Keccak256Transcript.from_proof(proof)
    for bad_n in (0, 31):
        with pytest.raises(hl.ArgumentError):
            hl.memcheck_verify(vp, bad_n, l, tr(), init=init)
        with pytest.raises(hl.ArgumentError):  # (refused before the prover param or the device is touched)
            hl.memcheck_prove(None, 1, 2, 3, l, hl.Keccak256Transcript(), init=init, num_vars=bad_n)
    for bad_l, image in ((0, None), (31, None), (0, [7]), (2, init), (4, init)):
        with pytest.raises(hl.ArgumentError):
            hl.memcheck_verify(vp, n, bad_l, tr(), init=image)
        with pytest.raises(hl.ArgumentError):
            hl.memcheck_prove(None, 1, 2, 3, bad_l, hl.Keccak256Transcript(), init=image, num_vars=n)
    with pytest.raises(hl.ArgumentError):  # 25 variables of memory with an image: the verifier would fold 2^25 words
        hl.memcheck_verify(vp, n, 25, tr(), init=init)
    with pytest.raises(hl.ArgumentError):  # a word of the image above 32 bits
        hl.memcheck_verify(vp, n, l, tr(), init=init[:-1] + [1 << 32])
    with pytest.raises(hl.ArgumentError):  # a missing column; raw pointers without num_vars
        hl.memcheck_prove(None, 1, None, 3, l, hl.Keccak256Transcript(), init=init, num_vars=n)
    with pytest.raises(hl.ArgumentError):
        hl.memcheck_prove(None, 1, 2, 3, l, hl.Keccak256Transcript(), init=init)
    # max(n, l) above the param: seven variables against the 6-variable param, either way
    with pytest.raises(hl.InvalidPcsParam):
        hl.memcheck_verify(vp, 7, l, tr(), init=init)
    with pytest.raises(hl.InvalidPcsParam):
        hl.memcheck_verify(vp, n, 7, tr(), init=init * 16)
    with pytest.raises(hl.InvalidPcsParam):
        hl.memcheck_verify(vp, n, 30, tr())
    # the same through ctypes: the library's own answers
    image = (C.c_uint32 * len(init))(*init)
    t = tr()
    assert lib.lh_memcheck_verify(vp.h, n, l, image, hl.Keccak256Transcript.from_proof(proof).p) == _ffi.LH_OK
    assert lib.lh_memcheck_verify(None, n, l, image, t.p) == _ffi.LH_ERR_ARG  # NULL param
    assert lib.lh_memcheck_verify(vp.h, n, l, image, None) == _ffi.LH_ERR_ARG  # NULL transcript
    for bad_n, bad_l, img in ((0, l, image), (31, l, image), (n, 0, image), (n, 25, image), (n, 0, None), (n, 31, None)):
        assert lib.lh_memcheck_verify(vp.h, bad_n, bad_l, img, t.p) == _ffi.LH_ERR_ARG, (bad_n, bad_l)
        assert (b"num_vars" if bad_n != n else b"mem_vars") in lib.lh_last_error()
    assert lib.lh_memcheck_verify(vp.h, n, 25, None, t.p) == _ffi.LH_ERR_INVALID_PCS_PARAM  # (legal without an image)
    assert lib.lh_memcheck_verify(vp.h, 7, l, image, t.p) == _ffi.LH_ERR_INVALID_PCS_PARAM
    assert lib.lh_memcheck_verify(vp.h, n, l, None, t.p) == _ffi.LH_ERR_INVALID_SNARK  # (NULL image: another statement)
    t = tr()
    # the prover's and the debug entry's, as far as they get without a device: NULL ctx, and never a crash on NULL lists
    trace = _ffi.lh_memcheck_trace()
    assert lib.lh_memcheck_prove(None, None, C.byref(trace), n, l, image, t.p) == _ffi.LH_ERR_ARG
    assert lib.lh_memcheck_prove(None, None, None, n, l, None, None) == _ffi.LH_ERR_ARG
    bad = C.c_int(0)
    assert lib.lh_debug_memcheck_witness(None, C.byref(trace), n, l, image, None, None, None, None, C.byref(bad)) == _ffi.LH_ERR_ARG
    assert lib.lh_debug_memcheck_witness(None, None, n, l, None, None, None, None, None, None) == _ffi.LH_ERR_ARG
    assert t.remaining() == len(proof), "refused before a byte is read"
