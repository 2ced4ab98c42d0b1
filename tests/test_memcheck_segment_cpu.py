"""CPU: memory checking in segments (lh_memcheck_prove_segment / lh_memcheck_verify_segment, hl.memcheck_verify_chain) - the
specification (tests/memcheck_segment_ref.py) against its golden proofs (tests/golden/memcheck_segment.json,
tests/golden/make_memcheck_segment.py), the host verifier on those proofs, on damaged ones and on three cheating provers',
the chain check, and the refusals that need no device."""
import ctypes as C
import json
import os
import re

import pytest

import logup_gkr_ref as lgr
import memcheck_ref as mcr
import memcheck_segment_ref as msr
from oracle.pyref import gkr as o_gkr, kzg as o_kzg
from oracle.pyref.transcript import Keccak256Transcript as OT

HERE = os.path.dirname(os.path.abspath(__file__))
FILE = json.load(open(os.path.join(HERE, "golden", "memcheck_segment.json")))
GOLDEN, CHAIN, FORGED = FILE["cases"], FILE["chain"], FILE["forgeries"]
PLAIN = json.load(open(os.path.join(HERE, "golden", "memcheck.json")))["cases"]
SS = [int(x, 16) for x in json.load(open(os.path.join(HERE, "golden", "lasso_tables.json")))["srs"]["ss"]]
CASES = list(msr.CASES)
CHAIN_WORDS = "memcheck chain: segment %d does not start where segment %d ends"


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


def point(rec):
    return None if rec is None else (int(rec[0], 16), int(rec[1], 16))


def verify(hl, vp, case, proof=None, **over):
    n, l = msr.CASES[case]
    a = dict(n=n, l=l)
    a.update(over)
    tr = hl.Keccak256Transcript.from_proof(proof_of(case) if proof is None else proof)
    return hl.memcheck_verify_segment(vp, a["n"], a["l"], tr), tr


# ------------------------------------------------------------------ 1. the specification
def test_the_cases_are_the_named_ones():
    assert list(GOLDEN) == CASES and len(CASES) == 8 and set(FORGED) == set(msr.FORGERIES) and len(FORGED) == 3
    assert msr.SMALL == [c for c in CASES if c != "mid"] and len(SS) == 6 and msr.CHAIN == (5, 5, 3) and len(CHAIN) == 3
    want = dict(one_var=(1, 1), small_mem=(5, 3), big_mem=(2, 4), zero_image=(4, 3), loads_only=(4, 3), one_cell=(4, 1),
                edges=(3, 2), mid=(13, 9))
    assert msr.CASES == want
    for case, (n, l) in msr.CASES.items():
        g = GOLDEN[case]
        assert (g["n"], g["l"]) == (n, l) and len(msr.case_image(case)) == 1 << l
        addr, rv, wv = msr.case_trace(case)
        assert len(addr) == len(rv) == len(wv) == 1 << n and max(addr) < 1 << l and max(rv + wv) < 1 << 32
    wit = lambda case: mcr.witness(*msr.case_trace(case), msr.case_image(case))
    # zero_image: iv commits to the identity - bit 3 of the mask (its repr is big-endian) - and the verifier returns None
    assert not any(msr.case_image("zero_image")) and int.from_bytes(proof_of("zero_image")[:32], "big") == 1 << msr.IV
    assert GOLDEN["zero_image"]["image_commitment"] is None and GOLDEN["zero_image"]["final_commitment"] is not None
    # loads_only: the memory ends as it began, and the two commitments are equal
    assert wit("loads_only")["fv"] == msr.case_image("loads_only")
    assert GOLDEN["loads_only"]["image_commitment"] == GOLDEN["loads_only"]["final_commitment"] is not None
    # big_mem: cells nobody touches keep iv and time 0
    w, touched, image = wit("big_mem"), set(msr.case_trace("big_mem")[0]), msr.case_image("big_mem")
    assert len(touched) < 16 and all(w["ft"][a] == 0 and w["fv"][a] == image[a] for a in range(16) if a not in touched)
    # one_cell: every operation on cell 0
    assert set(msr.case_trace("one_cell")[0]) == {0} and wit("one_cell")["rt"] == list(range(16))
    # edges: the edge words in the image and in the stores
    addr, rv, wv = msr.case_trace("edges")
    assert set(msr.EDGE_WORDS) <= set(wv) and set(msr.EDGE_WORDS[1:]) == set(msr.case_image("edges"))
    assert msr.EDGE_WORDS == [0, 1, 1 << 16, 1 << 31, (1 << 32) - 1]
    # the chain: every segment starts from the previous fv, and the commitments link
    traces, images = msr.chain_traces()
    for k, tr in enumerate(traces):
        assert mcr.witness(*tr, images[k])["fv"] == images[k + 1] != images[k]
        assert (CHAIN[k]["n"], CHAIN[k]["l"]) == msr.CHAIN[:2]
    assert CHAIN[0]["final_commitment"] == CHAIN[1]["image_commitment"] != CHAIN[1]["final_commitment"] == CHAIN[2]["image_commitment"]


@pytest.mark.parametrize("case", msr.SMALL)
def test_reference_proves_verifies_and_matches_golden(pp, case):
    n, l = msr.CASES[case]
    t = OT()
    fv = msr.prove(pp, *msr.case_trace(case), l, msr.case_image(case), t)
    assert fv == mcr.witness(*msr.case_trace(case), msr.case_image(case))["fv"]
    proof = t.into_proof()
    iv_c, fv_c = msr.verify(pp, n, l, OT(proof))
    assert proof.hex() == GOLDEN[case]["proof"], "the golden bytes are not what the specification produces now"
    assert (iv_c, fv_c) == (point(GOLDEN[case]["image_commitment"]), point(GOLDEN[case]["final_commitment"]))


def test_reference_reproduces_the_chain(pp):
    n, l, _ = msr.CHAIN
    traces, images = msr.chain_traces()
    proofs = []
    for k, trace in enumerate(traces):
        t = OT()
        msr.prove(pp, *trace, l, images[k], t)
        proofs.append(t.into_proof())
        assert proofs[-1].hex() == CHAIN[k]["proof"]
    first, last = msr.verify_chain(pp, l, [(n, p) for p in proofs], OT)
    assert (first, last) == (point(CHAIN[0]["image_commitment"]), point(CHAIN[2]["final_commitment"]))
    with pytest.raises(mcr.MemcheckError, match=CHAIN_WORDS % (1, 0)):
        msr.verify_chain(pp, l, [(n, proofs[0]), (n, proofs[2]), (n, proofs[1])], OT)


@pytest.mark.parametrize("name", list(msr.FORGERIES))
def test_reference_reproduces_and_refuses_the_forgeries(pp, name):
    n, l, image, trace, forge = msr.forgery(name)
    g = FORGED[name]
    assert (g["n"], g["l"], g["image"], (g["addr"], g["rv"], g["wv"])) == (n, l, image, tuple(trace))
    if name != "other_image":  # the honest prover has no proof of these traces
        with pytest.raises(mcr.MemcheckError, match="Invalid memory trace"):
            msr.prove(pp, *trace, l, image, OT())
    t = OT()
    msr.prove(pp, *trace, l, image, t, forge=forge)
    assert t.into_proof().hex() == g["proof"]
    with pytest.raises((mcr.MemcheckError, o_kzg.PcsError), match=msr.FORGERIES[name]):
        msr.verify(pp, n, l, OT(bytes.fromhex(g["proof"])))


def test_other_image_is_the_honest_commitment_block_with_one_commitment_replaced(pp):
    """the forged proof carries another image's commitment where the honest one carries that of [3, 9]; the seven others stay"""
    n, l, image, trace, forge = msr.forgery("other_image")
    t = OT()
    msr.prove(pp, *trace, l, image, t)
    honest, forged = t.into_proof(), bytes.fromhex(FORGED["other_image"]["proof"])
    at = 32 + 64 * msr.IV  # (no column of this trace is zero: eight points behind the mask)
    assert int.from_bytes(honest[:32], "big") == 0 and honest[:at] == forged[:at] and honest[at:at + 64] != forged[at:at + 64]
    assert honest[at + 64:32 + 64 * msr.NUM_POLYS] == forged[at + 64:32 + 64 * msr.NUM_POLYS]
    assert msr.verify(pp, n, l, OT(honest))[0] == o_kzg.commit(pp.trim(2), [3, 9, 0, 0]) != o_kzg.commit(pp.trim(2), [4, 9, 0, 0])


# ------------------------------------------------------------------ 2. the host verifier
@pytest.mark.parametrize("case", CASES)
def test_host_verifier_accepts_golden_and_returns_the_commitments(hl, vp, vp_mid, case):
    (iv_c, fv_c), tr = verify(hl, vp if case in msr.SMALL else vp_mid, case)
    assert tr.remaining() == 0
    assert (iv_c, fv_c) == (point(GOLDEN[case]["image_commitment"]), point(GOLDEN[case]["final_commitment"]))
    if case == "zero_image":
        assert iv_c is None and fv_c is not None, "the identity comes back as None - (0, 0) at the C ABI"
    if case == "loads_only":
        assert iv_c == fv_c is not None


def test_the_identity_is_zero_bytes_at_the_c_abi(hl, vp):
    from halo2_lasso_amd import _ffi
    lib = _ffi.load()
    n, l = msr.CASES["zero_image"]
    iv, fv = _ffi.lh_g1(), _ffi.lh_g1()
    C.memset(C.byref(iv), 0xAA, 64)
    t = hl.Keccak256Transcript.from_proof(proof_of("zero_image"))
    assert lib.lh_memcheck_verify_segment(vp.h, n, l, t.p, C.byref(iv), C.byref(fv)) == _ffi.LH_OK
    assert bytes(iv) == bytes(64) and bytes(fv) != bytes(64)
    # either output may be NULL
    t = hl.Keccak256Transcript.from_proof(proof_of("zero_image"))
    assert lib.lh_memcheck_verify_segment(vp.h, n, l, t.p, None, None) == _ffi.LH_OK
    # a refused proof writes neither
    C.memset(C.byref(iv), 0xAA, 64)
    t = hl.Keccak256Transcript.from_proof(proof_of("zero_image")[:-1])
    assert lib.lh_memcheck_verify_segment(vp.h, n, l, t.p, C.byref(iv), None) == _ffi.LH_ERR_INVALID_SNARK
    assert bytes(iv) == b"\xaa" * 64


@pytest.mark.parametrize("name", list(msr.FORGERIES))
def test_host_verifier_refuses_the_forgeries_where_it_should(hl, vp, name):
    """stale_init dies at the multiset identity, future_read at the range check on the fractions' roots; other_image is
    honest in every sum-check about the true image, and dies where the committed column is opened"""
    g = FORGED[name]
    words = {"other_image": "Invalid multilinear KZG open"}.get(name, msr.FORGERIES[name])
    with pytest.raises(hl.InvalidSnark, match=words):
        hl.memcheck_verify_segment(vp, g["n"], g["l"], hl.Keccak256Transcript.from_proof(bytes.fromhex(g["proof"])))


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
    n, l = msr.CASES[case]
    msr.verify(pp, n, l, OT(proof_of(case)))
    monkeypatch.undo()
    return at


@pytest.mark.parametrize("case", ["small_mem", "big_mem"])
def test_a_flipped_byte_in_each_section_is_invalid_snark(hl, vp, pp, monkeypatch, case):
    proof = proof_of(case)
    at = _sections(pp, case, monkeypatch)
    E = 32 * len(msr.OPENINGS)
    # (no column of these cases is zero: the mask is 0 and eight points follow it)
    assert int.from_bytes(proof[:32], "little") == 0 and at["grand product"] == 32 + 64 * msr.NUM_POLYS
    assert at["grand product"] < at["fractions"] < at["opening"] - E and at["opening"] < len(proof)
    where = {"mask": 31, "commitments": 32 + 3, "image commitment": 32 + 64 * msr.IV + 5, "final commitment": 32 + 64 * msr.FV + 40,
             "last commitment": at["grand product"] - 5, "grand product roots": at["grand product"] + 3,
             "grand product layers": at["fractions"] - 40, "fractions' roots": at["fractions"] + 3,
             "fractions' layers": at["opening"] - E - 40, "evaluations": at["opening"] - 29,
             "first evaluation": at["opening"] - E + 3, "image evaluation": at["opening"] - E + 32 * 4 + 7,
             "opening": at["opening"] + 3, "last quotient": len(proof) - 7}
    for name, pos in where.items():
        bad = bytearray(proof)
        bad[pos] ^= 4
        with pytest.raises(hl.InvalidSnark):
            verify(hl, vp, case, bytes(bad))
            pytest.fail("a flipped byte in the %s section verified" % name)


def test_trailing_truncated_and_other_shapes_are_invalid_snark(hl, vp):
    case = "small_mem"
    n, l = msr.CASES[case]
    proof = proof_of(case)
    verify(hl, vp, case)
    with pytest.raises(hl.InvalidSnark, match="trailing bytes"):
        verify(hl, vp, case, proof + b"\0")
    for cut in (proof[:-1], proof[:700], proof[:32], b""):  # a proof that ends early
        with pytest.raises(hl.InvalidSnark):
            verify(hl, vp, case, cut)
    for other in (dict(n=n - 1), dict(n=n + 1), dict(l=l - 1), dict(l=l + 1), dict(n=l, l=n)):
        with pytest.raises(hl.InvalidSnark):  # another shape
            verify(hl, vp, case, **other)
    with pytest.raises(hl.InvalidSnark):  # another case's proof of the same shape
        verify(hl, vp, "zero_image", proof_of("loads_only")[:-1])


def test_neither_verifier_takes_the_others_proof(hl, vp, vp_mid):
    for case, (n, l) in msr.CASES.items():  # the plain verifier on segment proofs: with the image public, and without one
        v = vp if case in msr.SMALL else vp_mid
        for init in (msr.case_image(case), None):
            with pytest.raises(hl.InvalidSnark):
                hl.memcheck_verify(v, n, l, hl.Keccak256Transcript.from_proof(proof_of(case)), init=init)
    assert len(PLAIN) == 10
    for case, (n, l, _) in mcr.CASES.items():  # the segment verifier on every proof of memcheck.json
        v = vp if case in mcr.SMALL else vp_mid
        with pytest.raises(hl.InvalidSnark):
            hl.memcheck_verify_segment(v, n, l, hl.Keccak256Transcript.from_proof(bytes.fromhex(PLAIN[case]["proof"])))


# ------------------------------------------------------------------ 3. the chain
def _chain():
    return [(c["n"], bytes.fromhex(c["proof"])) for c in CHAIN]


def test_the_chain_verifies(hl, vp):
    first, last = hl.memcheck_verify_chain(vp, msr.CHAIN[1], _chain())
    assert (first, last) == (point(CHAIN[0]["image_commitment"]), point(CHAIN[2]["final_commitment"]))
    assert hl.memcheck_verify_chain(vp, msr.CHAIN[1], _chain()[1:]) == (point(CHAIN[1]["image_commitment"]), last)


def test_a_chain_out_of_order_is_refused_with_the_chain_words(hl, vp):
    a, b, c = _chain()
    with pytest.raises(hl.InvalidSnark, match=CHAIN_WORDS % (1, 0)):
        hl.memcheck_verify_chain(vp, msr.CHAIN[1], [a, c, b])
    with pytest.raises(hl.InvalidSnark, match=CHAIN_WORDS % (2, 1)):
        hl.memcheck_verify_chain(vp, msr.CHAIN[1], [a, b, b])
    with pytest.raises(hl.InvalidSnark, match=CHAIN_WORDS % (1, 0)):
        hl.memcheck_verify_chain(vp, msr.CHAIN[1], [a, c])
    with pytest.raises(hl.InvalidSnark) as e:  # a damaged segment is its own error, not the chain's
        hl.memcheck_verify_chain(vp, msr.CHAIN[1], [a, (b[0], b[1][:-1]), c])
    assert "memcheck chain" not in str(e.value)


def test_segments_of_different_nv_are_an_argument_error(hl, vp):
    a, b, c = _chain()
    n, l, _ = msr.CHAIN
    with pytest.raises(hl.ArgumentError, match="memcheck chain"):  # (LH_ERR_ARG's exception; refused before a segment is verified)
        hl.memcheck_verify_chain(vp, l, [a, (n + 1, b[1]), c])
    # max(n, l) is what counts: fewer operations over the same memory keep nv, and fail only as proofs
    with pytest.raises(hl.InvalidSnark):
        hl.memcheck_verify_chain(vp, l, [a, (n - 1, b[1]), c])
    with pytest.raises(hl.ArgumentError):
        hl.memcheck_verify_chain(vp, l, [])
    with pytest.raises(hl.ArgumentError):
        hl.memcheck_verify_chain(vp, l, [a, (0, b[1])])


# ------------------------------------------------------------------ 4. refusals that need no device
def test_symbols_are_present_in_every_layer():
    from halo2_lasso_amd import _ffi
    lib = _ffi.load()
    root = os.path.dirname(HERE)
    header = open(os.path.join(root, "include", "lasso_hip.h")).read()
    sys_rs = open(os.path.join(root, "bindings", "rust", "src", "sys.rs")).read()
    for sym in ("lh_memcheck_replay", "lh_memcheck_prove_segment", "lh_memcheck_verify_segment"):
        assert hasattr(lib, sym) and sym in _ffi.SIGNATURES and re.search(r"lh_status %s\(" % sym, header)
        assert re.search(r"pub fn %s\(" % sym, sys_rs)
    # the fourth new name is the operations' struct: a type, so not in the library
    assert re.search(r"typedef struct lh_memcheck_ops \{\s*const uint32_t \*d_addr, \*d_store, \*d_val;", header)
    assert [f[0] for f in _ffi.lh_memcheck_ops._fields_] == ["d_addr", "d_store", "d_val"]
    assert re.search(r"pub struct lh_memcheck_ops \{ pub d_addr: \*const u32, pub d_store: \*const u32, pub d_val: \*const u32 \}", sys_rs)


def test_argument_refusals(hl, vp):
    from halo2_lasso_amd import _ffi
    lib = _ffi.load()
    case = "small_mem"
    n, l = msr.CASES[case]
    proof = proof_of(case)
    tr = lambda: hl.Keccak256Transcript.from_proof(proof)
    for bad_n in (0, 31):
        with pytest.raises(hl.ArgumentError, match="num_vars"):
            hl.memcheck_verify_segment(vp, bad_n, l, tr())
        with pytest.raises(hl.ArgumentError):  # (refused before the prover param or the device is touched)
            hl.memcheck_prove_segment(None, 1, 2, 3, l, 4, hl.Keccak256Transcript(), num_vars=bad_n)
        with pytest.raises(hl.ArgumentError):
            hl.memcheck_replay(None, 1, 2, 3, l, num_vars=bad_n)
    for bad_l in (0, 31):
        with pytest.raises(hl.ArgumentError, match="mem_vars"):
            hl.memcheck_verify_segment(vp, n, bad_l, tr())
        with pytest.raises(hl.ArgumentError):
            hl.memcheck_prove_segment(None, 1, 2, 3, bad_l, 4, hl.Keccak256Transcript(), num_vars=n)
        with pytest.raises(hl.ArgumentError):
            hl.memcheck_replay(None, 1, 2, 3, bad_l, num_vars=n)
    with pytest.raises(hl.ArgumentError):  # a segment without its image
        hl.memcheck_prove_segment(None, 1, 2, 3, l, None, hl.Keccak256Transcript(), num_vars=n)
    with pytest.raises(hl.ArgumentError):  # a missing column; raw pointers without num_vars
        hl.memcheck_prove_segment(None, 1, None, 3, l, 4, hl.Keccak256Transcript(), num_vars=n)
    with pytest.raises(hl.ArgumentError):
        hl.memcheck_replay(None, 1, None, 3, l, num_vars=n)
    with pytest.raises(hl.ArgumentError):
        hl.memcheck_replay(None, 1, 2, 3, l)
    # 25 variables of memory: nothing is folded, so the argument check accepts it and only the param is too small - the
    # plain entry with an image refuses the shape itself
    with pytest.raises(hl.InvalidPcsParam):
        hl.memcheck_verify_segment(vp, n, 25, tr())
    with pytest.raises(hl.ArgumentError):
        hl.memcheck_verify(vp, n, 25, tr(), init=msr.case_image(case))
    with pytest.raises(hl.InvalidPcsParam):  # max(n, l) above the param, either way
        hl.memcheck_verify_segment(vp, 7, l, tr())
    with pytest.raises(hl.InvalidPcsParam):
        hl.memcheck_verify_segment(vp, n, 30, tr())
    # the same through ctypes: the library's own answers
    t = tr()
    iv = _ffi.lh_g1()
    assert lib.lh_memcheck_verify_segment(vp.h, n, l, hl.Keccak256Transcript.from_proof(proof).p, C.byref(iv), None) == _ffi.LH_OK
    assert lib.lh_memcheck_verify_segment(None, n, l, t.p, None, None) == _ffi.LH_ERR_ARG  # NULL param
    assert lib.lh_memcheck_verify_segment(vp.h, n, l, None, None, None) == _ffi.LH_ERR_ARG  # NULL transcript
    for bad_n, bad_l in ((0, l), (31, l), (n, 0), (n, 31)):
        assert lib.lh_memcheck_verify_segment(vp.h, bad_n, bad_l, t.p, None, None) == _ffi.LH_ERR_ARG, (bad_n, bad_l)
        assert (b"num_vars" if bad_n != n else b"mem_vars") in lib.lh_last_error()
    assert lib.lh_memcheck_verify_segment(vp.h, n, 25, t.p, None, None) == _ffi.LH_ERR_INVALID_PCS_PARAM
    assert lib.lh_memcheck_verify(vp.h, n, 25, (C.c_uint32 * 8)(), t.p) == _ffi.LH_ERR_ARG
    # the device entries, as far as they get without a device: the shape, then the NULL ctx, and never a crash on NULLs
    trace, ops = _ffi.lh_memcheck_trace(), _ffi.lh_memcheck_ops()
    assert lib.lh_memcheck_prove_segment(None, None, C.byref(trace), n, l, None, None, t.p) == _ffi.LH_ERR_ARG
    assert lib.lh_memcheck_prove_segment(None, None, None, n, l, None, None, None) == _ffi.LH_ERR_ARG
    assert lib.lh_memcheck_prove_segment(None, None, None, n, 31, None, None, None) == _ffi.LH_ERR_ARG
    assert b"mem_vars" in lib.lh_last_error()
    assert lib.lh_memcheck_prove_segment(None, None, None, n, 25, None, None, None) == _ffi.LH_ERR_ARG
    assert b"mem_vars" not in lib.lh_last_error(), "25 variables pass the shape check: the NULL ctx is what is refused"
    assert lib.lh_memcheck_replay(None, C.byref(ops), n, l, None, None, None, None) == _ffi.LH_ERR_ARG
    assert lib.lh_memcheck_replay(None, None, n, l, None, None, None, None) == _ffi.LH_ERR_ARG
    assert lib.lh_memcheck_replay(None, None, 0, l, None, None, None, None) == _ffi.LH_ERR_ARG
    assert b"num_vars" in lib.lh_last_error()
    assert t.remaining() == len(proof), "refused before a byte is read"
