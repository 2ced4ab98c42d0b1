"""CPU: Nova folding and relaxed Spartan (lh_nova_fold_verify / lh_spartan_verify_relaxed) - the specification
(tests/nova_ref.py) against its golden file (tests/golden/nova.json, tests/golden/make_nova.py: the six-variable cases are
pinned there by length and SHA-256, made here once by the specification and shared) and against the dense statement; the host
fold verifier and the relaxed verifier on those bytes, on the cheating prover's and on damaged ones; the refusals that need no
device; the exported symbols."""
import ctypes as C
import hashlib
import json
import os
import re

import pytest

import logup_gkr_ref as lgr
import nova_ref as nv
import spark_ref as spr
import spartan_ref as spa
from oracle.pyref import kzg as o_kzg, sum_check as o_sc
from oracle.pyref.field import R_MOD as P
from oracle.pyref.transcript import Keccak256Transcript as OT

HERE = os.path.dirname(os.path.abspath(__file__))
FILE = json.load(open(os.path.join(HERE, "golden", "nova.json")))
GOLDEN, FORGED = FILE["cases"], FILE["forgeries"]
SS = [int(x, 16) for x in json.load(open(os.path.join(HERE, "golden", "lasso_tables.json")))["srs"]["ss"]]
CASES = list(nv.CASES)


@pytest.fixture(scope="module")
def vp(hl):
    return hl.MultilinearKzgVerifierParams.setup(SS)


@pytest.fixture(scope="module")
def vp_mid(hl):
    return hl.MultilinearKzgVerifierParams.setup(lgr.mid_ss())


_MADE = {}


def _pp():
    if "pp" not in _MADE:
        _MADE["pp"] = o_kzg.setup(SS)
    return _MADE["pp"]


@pytest.fixture(scope="module")
def pp():
    return _pp()


def _key(case):
    if ("key", case) not in _MADE:
        _MADE["key", case] = spa.commit(_pp(), nv.case_instance(case)[0], nv.CASES[case][1])
    return _MADE["key", case]


def _run(case, forge=None):
    """the specification's run of a small case, once"""
    if ("run", case, forge) not in _MADE:
        _MADE["run", case, forge] = nv.run(_pp(), _key(case), case, forge=forge)
    return _MADE["run", case, forge]


def _is(rec, prefix, data):
    return (len(data), hashlib.sha256(data).hexdigest()) == (rec[prefix + "bytes"], rec[prefix + "sha256"])


def steps(case):
    """-> (key blob, [per step a dict: step, a, b, blob, proof]): stored in full (`mid`) or made by the specification and
    equal to the file in length and digest"""
    if ("steps", case) in _MADE:
        return _MADE["steps", case]
    g = GOLDEN[case]
    if case in nv.SMALL:
        key_blob, records = _key(case).blob, _run(case)[1]
    else:
        key_blob = bytes.fromhex(g["key"])
        records = [dict(s, **{k: bytes.fromhex(s[k]) for k in ("blob", "proof") if k in s}) for s in g["steps"]]
    assert _is(g, "key_", key_blob), "%s: the golden key is not what the specification produces now" % case
    assert len(records) == len(g["steps"])
    for rec, s in zip(records, g["steps"]):
        assert rec["step"] == s["step"] and all(rec[k] == s[k] for k in ("a", "b") if k in s)
        for part in ("blob", "proof"):
            if part + "_bytes" in s:
                assert _is(s, part + "_", rec[part]), "%s: a golden %s is not what the specification produces now" % (case, part)
    _MADE["steps", case] = key_blob, records
    return _MADE["steps", case]


def blobs(case):
    return [r["blob"] for r in steps(case)[1] if r["step"] != "prove"]


def final(case):
    """-> (key blob, the instance blob that is proved, the relaxed proof)"""
    key_blob, records = steps(case)
    last = records[-1]
    assert last["step"] == "prove"
    return key_blob, blobs(case)[last["a"]], last["proof"]


def forged(name):
    """-> (key blob, the blob the relaxed verifier is given, the proof) of a forgery, by the generator's own recipe"""
    if ("forged", name) not in _MADE:
        import importlib.util
        spec = importlib.util.spec_from_file_location("make_nova", os.path.join(HERE, "golden", "make_nova.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        key_blob, blob, proof = mod.forgery(_pp(), name)
        g = FORGED[name]
        assert _is(g, "blob_", blob) and _is(g, "proof_", proof), "%s: the golden forgery is not what the specification produces now" % name
        _MADE["forged", name] = key_blob, blob, proof
    return _MADE["forged", name]


def verify(hl, vp, case, **over):
    n, l, p = nv.CASES[case]
    key_blob, blob, proof = final(case)
    a = dict(n=n, l=l, commitment=key_blob, instance=blob, p=p, proof=proof)
    a.update(over)
    hl.spartan_verify_relaxed(vp, a["n"], a["l"], a["commitment"], a["instance"], a["p"], a["proof"])


# ------------------------------------------------------------------ 1. the specification
def test_the_cases_are_the_named_ones():
    assert set(GOLDEN) == set(nv.CASES) == set(nv.SCHEDULES) and len(nv.CASES) == 8 and set(FORGED) == set(nv.FORGERIES)
    assert set(nv.FORGERIES) == {"bad_T", "bad_vE", "other_input"} and all(FORGED[f]["case"] == nv.FORGERY_CASE == "chain" for f in FORGED)
    assert nv.SMALL == [c for c in CASES if c != "mid"] and len(SS) == 6
    assert nv.CASES == {"tiny": (1, 2, 1), "chain": (3, 3, 2), "two_relaxed": (3, 3, 2), "self_fold": (3, 3, 1), "fresh_relaxed": (3, 3, 2),
                        "tall": (2, 4, 3), "full_public": (3, 3, 4), "mid": (12, 10, 5)}
    for case in CASES:
        n, l, p = nv.CASES[case]
        g = GOLDEN[case]
        assert (g["n"], g["l"], g["p"]) == (n, l, p)
        assert [(s["step"],) + tuple(s[k] for k in ("a", "b") if k in s) for s in g["steps"]] == \
            [(s[0],) + tuple(s[1:]) if s[0] != "fresh" else ("fresh",) for s in nv.SCHEDULES[case]]
    # what is stored in full: the one case the specification takes a minute to make
    assert [c for c in CASES if "key" in GOLDEN[c]] == ["mid"]
    assert [c for c in CASES if any("proof" in s or "blob" in s for s in GOLDEN[c]["steps"])] == ["mid"]
    folds = lambda case: [s for s in GOLDEN[case]["steps"] if s["step"] == "fold"]
    # a fold's proof is the T block alone: 96 bytes; self_fold's T is zero: the mask element alone, and C_E stays the identity
    assert all(s["proof_bytes"] == 96 for c in CASES if c != "self_fold" for s in folds(c))
    assert [s["proof_bytes"] for s in folds("self_fold")] == [32]
    assert [len(folds(c)) for c in ("tiny", "chain", "two_relaxed", "self_fold", "fresh_relaxed", "mid")] == [1, 3, 3, 1, 0, 2]
    # chain: a running instance takes three fresh ones; two_relaxed: the last fold's second input is itself folded
    assert [(s["a"], s["b"]) for s in folds("chain")] == [(0, 1), (4, 2), (5, 3)]
    assert [(s["a"], s["b"]) for s in folds("two_relaxed")] == [(0, 1), (2, 3), (4, 5)]
    assert nv.CASES["tall"][1] > nv.CASES["tall"][0] and nv.CASES["full_public"][2] == 1 << (nv.CASES["full_public"][1] - 1)


@pytest.mark.parametrize("case", nv.SMALL)
def test_reference_reproduces_the_golden(pp, case):
    n, l, p = nv.CASES[case]
    inst, assigns = nv.case_instance(case)
    key = _key(case)
    key_blob, records = steps(case)  # (made by the specification: lengths and digests are the file's)
    slots, _ = _run(case)
    every = blobs(case)
    for (w, x) in assigns:
        assert x[0] == 1 and spa.satisfied(inst, w, x, l) == 0, "a fresh assignment satisfies the plain dense statement"
    for (U, (w, E)), blob in zip(slots, every):
        assert nv.relaxed_satisfied(inst, w, E, U.x, l) == 0, "the dense relaxed relation"
        assert U.cw == o_kzg.commit(pp.trim(l - 1), w) and U.ce == (o_kzg.commit(pp.trim(l), E) if E is not None else None)
        assert U.blob == blob and len(blob) == 32 + 64 * ((U.cw is not None) + (U.ce is not None)) + 32 * p
        assert int.from_bytes(blob[:32], "big") == (U.cw is None) + 2 * (U.ce is None)
        back = nv.read_instance(blob, p)
        assert (back.cw, back.ce, back.x) == (U.cw, U.ce, U.x)
    for rec in records:
        if rec["step"] == "fold":  # the fold verifier returns the prover's blob
            assert nv.fold_verify(n, l, p, key_blob, every[rec["a"]], every[rec["b"]], OT(rec["proof"])) == rec["blob"]
        if rec["step"] == "prove":
            nv.verify_relaxed(pp, n, l, p, key_blob, every[rec["a"]], OT(rec["proof"]))
    if case == "self_fold":
        U, (w, E) = slots[1]
        assert U.ce is None and not any(E) and U.x[0] not in (0, 1) and records[1]["proof"] == b"\0" * 31 + b"\1"
    if case == "fresh_relaxed":
        assert slots[0][0].ce is None and slots[0][1][1] is None
    if case in ("chain", "two_relaxed"):
        assert all(any(W[1]) for U, W in slots[4:]), "the cross terms are not zero"


def test_an_unsatisfying_input_is_refused_by_the_specification(pp):
    case = "chain"
    key = _key(case)
    slots, _ = _run(case)
    (U1, (w1, _)), (U2, (w2, _)) = slots[0], slots[1]
    bad = list(w1)
    bad[0] = (bad[0] + 1) % P
    with pytest.raises(nv.NovaError, match=r"input 1 does not satisfy \d of the 2\^3 constraints"):
        nv.fold(pp, key, U1, (bad, None), U2, (w2, None), OT())
    with pytest.raises(nv.NovaError, match=r"input 2 does not satisfy \d of the 2\^3 constraints"):
        nv.fold(pp, key, U2, (w2, None), U1, (bad, None), OT())
    (U, (w, E)) = slots[4]
    worse = list(E)
    worse[1] = (worse[1] + 1) % P
    with pytest.raises(nv.NovaError, match=r"input 2 does not satisfy 1 of the 2\^3 constraints"):
        nv.fold(pp, key, U1, (w1, None), U, (w, worse), OT())


@pytest.mark.parametrize("name", list(nv.FORGERIES))
def test_reference_refuses_the_forgeries(pp, name):
    n, l, p = nv.CASES[nv.FORGERY_CASE]
    key_blob, blob, proof = forged(name)
    with pytest.raises(spa.SpartanError, match=nv.FORGERIES[name]):
        nv.verify_relaxed(pp, n, l, p, key_blob, blob, OT(proof))
    honest_blob, honest_proof = final(nv.FORGERY_CASE)[1:]
    if name == "other_input":  # the honest proof, against the instance another U2 folds into
        assert proof == honest_proof and blob != honest_blob
    if name == "bad_vE":
        assert blob == honest_blob and proof != honest_proof
    if name == "bad_T":
        assert blob != honest_blob


# ------------------------------------------------------------------ 2. the host verifiers
@pytest.mark.parametrize("case", CASES)
def test_host_verifiers_accept_golden(hl, vp, vp_mid, case):
    n, l, p = nv.CASES[case]
    key_blob, records = steps(case)
    every = blobs(case)
    for rec in records:
        if rec["step"] == "fold":
            assert hl.nova_fold_verify(n, l, key_blob, every[rec["a"]], every[rec["b"]], rec["proof"]) == rec["blob"]
    verify(hl, vp if case in nv.SMALL else vp_mid, case)


@pytest.mark.parametrize("name", list(nv.FORGERIES))
def test_host_verifier_refuses_the_forgeries(hl, vp, name):
    n, l, p = nv.CASES[nv.FORGERY_CASE]
    key_blob, blob, proof = forged(name)
    with pytest.raises(hl.InvalidSnark, match="spartan: .*" + nv.FORGERIES[name]):
        hl.spartan_verify_relaxed(vp, n, l, key_blob, blob, p, proof)
    if name == "other_input":  # the host fold verifier returns that instance for the other U2
        every, last = blobs(nv.FORGERY_CASE), [r for r in steps(nv.FORGERY_CASE)[1] if r["step"] == "fold"][-1]
        assert hl.nova_fold_verify(n, l, key_blob, every[last["a"]], every[1], last["proof"]) == blob
    if name == "bad_T":  # the damaged fold verifies: nothing in a fold is checked
        _, records = _run(nv.FORGERY_CASE, "bad_T")
        every, last = [r["blob"] for r in records if r["step"] != "prove"], [r for r in records if r["step"] == "fold"][-1]
        assert hl.nova_fold_verify(n, l, key_blob, every[last["a"]], every[last["b"]], last["proof"]) == blob


def _sections(pp, case, monkeypatch):
    """where the sections of a golden relaxed proof begin: the specification's verifier is asked, at the entry of its pieces"""
    at = {}

    def spy(name, fn, tr_arg):
        def wrapped(*a, **k):
            at.setdefault(name, []).append(a[tr_arg].pos)
            return fn(*a, **k)
        return wrapped

    monkeypatch.setattr(o_sc, "verify", spy("sum-check", o_sc.verify, 4))
    monkeypatch.setattr(o_kzg, "batch_verify", spy("opening", o_kzg.batch_verify, 5))
    monkeypatch.setattr(spr, "verify", spy("spark", spr.verify, 7))
    n, l, p = nv.CASES[case]
    key_blob, blob, proof = final(case)
    nv.verify_relaxed(pp, n, l, p, key_blob, blob, OT(proof))
    monkeypatch.undo()
    return at


@pytest.mark.parametrize("case", ["chain", "tall", "fresh_relaxed"])
def test_a_flipped_byte_in_each_section_is_invalid_snark(hl, vp, pp, monkeypatch, case):
    n, l, p = nv.CASES[case]
    key_blob, blob, proof = final(case)
    at = _sections(pp, case, monkeypatch)
    # no w block: the outer sum-check at once, l rounds of 4, four values; the inner: l rounds of 3, four values; the opening
    # of w; the opening of E unless C_E is the identity; the three Spark openings
    outer, inner = at["sum-check"][0], at["sum-check"][1]
    opens, sparks = at["opening"], at["spark"]
    relaxed = case != "fresh_relaxed"
    assert outer == 0 and inner == 32 * (4 * l + 4) and opens[0] == inner + 32 * (3 * l + 4) and len(sparks) == 3
    # (spark_ref.verify opens too: the first 1 + relaxed openings are this argument's own)
    assert (int.from_bytes(blob[:32], "big") == 0) == relaxed and len([o for o in opens if o < sparks[0]]) == 1 + relaxed
    where = {"outer rounds": 3, "outer last round": inner - 32 * 4 - 5, "vA": inner - 32 * 4 + 1, "vC": inner - 32 - 2, "vE": inner - 2,
             "inner rounds": inner + 7, "eA": opens[0] - 32 * 4 + 3, "eC": opens[0] - 32 - 4, "e_w": opens[0] - 3,
             "opening of w": opens[0] + 9, "last quotient before Spark": sparks[0] - 6, "Spark A": sparks[0] + 40,
             "Spark B": sparks[1] + 40, "Spark C": sparks[2] + 40, "last quotient": len(proof) - 7}
    if relaxed:
        where.update({"w quotient": opens[1] - 6, "opening of E": opens[1] + 9})
    for name, pos in where.items():
        bad = bytearray(proof)
        bad[pos] ^= 4
        with pytest.raises(hl.InvalidSnark, match="spartan: "):
            verify(hl, vp, case, proof=bytes(bad))
            pytest.fail("a flipped byte in the %s section verified" % name)
    # the instance blob: its mask, each point, each element of x
    points = 2 if relaxed else 1
    for pos in [31] + [32 + 64 * i + 5 for i in range(points)] + [32 + 64 * i + 32 + 7 for i in range(points)] + \
            [32 + 64 * points + 32 * i + 31 for i in range(p)]:
        bad = bytearray(blob)
        bad[pos] ^= 4
        with pytest.raises(hl.InvalidSnark, match="spartan: "):
            verify(hl, vp, case, instance=bytes(bad))
            pytest.fail("a flipped byte at %d of the instance verified" % pos)
    # the key blob: in each matrix's part its mask, a point
    parts = spa.split_key(key_blob)
    start = 0
    for b in parts:
        for pos in (start + 31, start + 32 + 3, start + len(b) - 2):
            bad = bytearray(key_blob)
            bad[pos] ^= 4
            with pytest.raises(hl.InvalidSnark, match="spartan: "):
                verify(hl, vp, case, commitment=bytes(bad))
                pytest.fail("a flipped byte at %d of the key verified" % pos)
        start += len(b)


def test_other_inputs_lengths_and_shapes_are_invalid_snark(hl, vp):
    case = "chain"
    n, l, p = nv.CASES[case]
    key_blob, blob, proof = final(case)
    verify(hl, vp, case)
    # another p: the blob no longer has the length the statement says
    for other in (1, 3, 4):
        with pytest.raises(hl.InvalidSnark, match="spartan: malformed instance"):
            verify(hl, vp, case, p=other)
    # another instance of the same key, another key
    with pytest.raises(hl.InvalidSnark):
        verify(hl, vp, case, instance=blobs(case)[5])
    with pytest.raises(hl.InvalidSnark):
        verify(hl, vp, case, commitment=steps("two_relaxed")[0])
    with pytest.raises(hl.InvalidSnark, match="spartan: trailing bytes"):
        verify(hl, vp, case, proof=proof + b"\0")
    for cut in (proof[:-1], proof[:2000], proof[:700], proof[:40], b""):  # a proof that ends early
        with pytest.raises(hl.InvalidSnark):
            verify(hl, vp, case, proof=cut)
    # a malformed instance: too short, too long, a mask out of range, a mask that wants fewer points than follow, a point off
    # the curve, an element that is no field element
    off_curve = bytearray(blob)
    off_curve[32 + 63] ^= 1
    no_element = blob[:-32] + b"\xff" * 32
    for bad in (blob[:-1], blob + b"\0", blob[:-32], blob + b"\0" * 32, b"\0" * 31 + b"\x04" + blob[32:], b"\0" * 31 + b"\x01" + blob[32:],
                bytes(off_curve), no_element, b"\1", b""):
        with pytest.raises(hl.InvalidSnark, match="spartan: malformed instance"):
            verify(hl, vp, case, instance=bad)
    parts = spa.split_key(key_blob)
    for bad in (key_blob[:-1], key_blob + b"\0", parts[0] + parts[1], b"\0" * 31 + b"\x80" + key_blob[32:], b""):
        with pytest.raises(hl.InvalidSnark, match="spartan: malformed"):
            verify(hl, vp, case, commitment=bad)
    for other in (dict(n=n - 1), dict(n=n + 1), dict(l=l + 1), dict(l=l - 1)):
        with pytest.raises(hl.InvalidSnark):  # another shape
            verify(hl, vp, case, **other)
    # fresh_relaxed: C_E is the identity, so vE must be zero - a blob that says "identity" for chain's proof is refused
    with pytest.raises(hl.InvalidSnark):
        verify(hl, vp, case, instance=b"\0" * 31 + b"\x02" + blob[32:96] + blob[160:])


def test_the_fold_verifier_refuses_malformed_input(hl):
    case = "chain"
    n, l, p = nv.CASES[case]
    key_blob, records = steps(case)
    every = blobs(case)
    rec = [r for r in records if r["step"] == "fold"][-1]
    b1, b2, proof = every[rec["a"]], every[rec["b"]], rec["proof"]
    fv = lambda **o: hl.nova_fold_verify(o.get("n", n), o.get("l", l), o.get("key", key_blob), o.get("b1", b1), o.get("b2", b2),
                                         o.get("proof", proof))
    assert fv() == rec["blob"]
    with pytest.raises(hl.InvalidSnark, match="nova: trailing bytes"):
        fv(proof=proof + b"\0")
    for cut in (proof[:-1], proof[:32], proof[:31], b""):
        with pytest.raises(hl.InvalidSnark, match="nova: "):
            fv(proof=cut)
    with pytest.raises(hl.InvalidSnark, match="nova: "):  # a mask out of range in the T block
        fv(proof=b"\0" * 31 + b"\x02" + proof[32:])
    for bad in (b1[:-1], b1 + b"\0", b"\0" * 31 + b"\x04" + b1[32:], b"\1", b""):
        with pytest.raises(hl.InvalidSnark, match="nova: malformed instance"):
            fv(b1=bad)
        with pytest.raises(hl.InvalidSnark, match="nova: malformed instance"):
            fv(b2=bad)
    with pytest.raises(hl.InvalidSnark, match="nova: the two instances have different numbers of public inputs"):
        fv(b2=b2 + b"\0" * 32)
    with pytest.raises(hl.InvalidSnark, match="nova: the two instances have different numbers of public inputs"):
        fv(b1=b1[:-32])
    with pytest.raises(hl.InvalidSnark, match="nova: malformed instance"):  # five public inputs in a half of four
        fv(b1=b1 + b"\0" * 96, b2=b2 + b"\0" * 96)
    parts = spa.split_key(key_blob)
    for bad in (key_blob[:-1], key_blob + b"\0", parts[0] + parts[1], b""):
        with pytest.raises(hl.InvalidSnark, match="^nova: malformed (key|commitment)"):
            fv(key=bad)
    # every part of the statement moves r: another key, another first input, a flipped byte of x -> another folded instance
    assert fv(key=steps("two_relaxed")[0]) != rec["blob"]
    assert fv(b1=every[0]) != rec["blob"]
    flipped = bytearray(b2)
    flipped[-1] ^= 1
    assert fv(b2=bytes(flipped)) != rec["blob"]
    assert fv(n=n + 1) != rec["blob"]


# ------------------------------------------------------------------ 3. refusals that need no device, the exported symbols
def test_argument_refusals_and_symbols(hl, vp):
    from halo2_lasso_amd import _ffi
    lib = _ffi.load()
    root = os.path.dirname(HERE)
    header = open(os.path.join(root, "include", "lasso_hip.h")).read()
    rust = open(os.path.join(root, "bindings", "rust", "src", "sys.rs")).read()
    symbols = ("lh_nova_instance", "lh_nova_fold", "lh_nova_fold_verify", "lh_spartan_prove_relaxed", "lh_spartan_verify_relaxed",
               "lh_debug_nova_spmv2", "lh_debug_nova_cross_term", "lh_debug_nova_fold")
    for sym in symbols:
        assert hasattr(lib, sym) and sym in _ffi.SIGNATURES and re.search(r"lh_status %s\(" % sym, header), sym
        assert re.search(r"pub fn %s\(" % sym, rust), sym
    assert "#define LH_NOVA_INSTANCE_BYTES(num_public) (160 + 32 * (size_t)(num_public))\n" in header
    assert hl.nova_instance_bytes(3) == 160 + 96
    for name in ("nova_instance", "nova_fold", "nova_fold_verify", "spartan_prove_relaxed", "spartan_verify_relaxed", "nova_spmv2",
                 "nova_cross_term", "nova_fold_vectors"):
        assert callable(getattr(hl, name))
    makefile = open(os.path.join(root, "halo2-lasso_amd", "csrc", "Makefile")).read()
    assert "kernels_nova.o" in makefile and " nova.o" in makefile

    case = "chain"
    n, l, p = nv.CASES[case]
    key_blob, blob, proof = final(case)
    for bad in (dict(n=0), dict(n=31), dict(l=1, p=1), dict(l=25), dict(p=0), dict(p=5), dict(commitment=None), dict(proof=None),
                dict(instance=None)):
        with pytest.raises(hl.ArgumentError):
            verify(hl, vp, case, **bad)
    with pytest.raises(hl.InvalidPcsParam):
        verify(hl, vp, case, n=7)
    with pytest.raises(hl.InvalidPcsParam):
        verify(hl, vp, case, l=7)
    for bad in ((0, l), (31, l), (n, 1), (n, 25)):
        with pytest.raises(hl.ArgumentError):
            hl.nova_fold_verify(bad[0], bad[1], key_blob, blob, blob, b"")
    with pytest.raises(hl.ArgumentError):
        hl.nova_fold_verify(n, l, None, blob, blob, b"")
    # the same through ctypes: the library's own answers
    tr = lambda: hl.Keccak256Transcript.from_proof(proof)
    arr = lambda b: (C.c_uint8 * len(b)).from_buffer_copy(b)
    cm, ib = arr(key_blob), arr(blob)
    t = tr()
    call = lib.lh_spartan_verify_relaxed
    assert call(vp.h, n, l, cm, len(key_blob), ib, len(blob), p, tr().p) == _ffi.LH_OK
    assert call(None, n, l, cm, len(key_blob), ib, len(blob), p, t.p) == _ffi.LH_ERR_ARG
    assert call(vp.h, n, l, None, len(key_blob), ib, len(blob), p, t.p) == _ffi.LH_ERR_ARG
    assert call(vp.h, n, l, cm, len(key_blob), None, len(blob), p, t.p) == _ffi.LH_ERR_ARG
    assert call(vp.h, n, l, cm, len(key_blob), ib, len(blob), p, None) == _ffi.LH_ERR_ARG
    for bn, bl, bp, word in ((0, l, p, b"num_vars"), (31, l, p, b"num_vars"), (n, 1, 1, b"dim_vars"), (n, 25, p, b"dim_vars"),
                             (n, l, 0, b"num_public"), (n, l, 5, b"num_public")):
        assert call(vp.h, bn, bl, cm, len(key_blob), ib, len(blob), bp, t.p) == _ffi.LH_ERR_ARG, (bn, bl, bp)
        assert word in lib.lh_last_error()
    assert call(vp.h, 7, l, cm, len(key_blob), ib, len(blob), p, t.p) == _ffi.LH_ERR_INVALID_PCS_PARAM
    assert call(vp.h, n, l, cm, len(key_blob), ib, len(blob) - 1, p, t.p) == _ffi.LH_ERR_INVALID_SNARK
    assert b"spartan: malformed instance" in lib.lh_last_error()
    assert call(vp.h, n, l, cm, len(key_blob) - 1, ib, len(blob), p, t.p) == _ffi.LH_ERR_INVALID_SNARK
    assert b"spartan: malformed" in lib.lh_last_error()
    assert t.remaining() == len(proof), "refused before a byte is read"
    # the fold verifier: NULLs, a buffer without room
    _, records = steps(case)
    rec = [r for r in records if r["step"] == "fold"][0]
    every = blobs(case)
    b1, b2 = arr(every[rec["a"]]), arr(every[rec["b"]])
    out, room = (C.c_uint8 * 512)(), C.c_size_t(512)
    ft = lambda: hl.Keccak256Transcript.from_proof(rec["proof"])
    fold = lib.lh_nova_fold_verify
    assert fold(n, l, cm, len(key_blob), b1, len(b1), b2, len(b2), out, C.byref(room), ft().p) == _ffi.LH_OK
    assert bytes(out[:room.value]) == rec["blob"]
    room = C.c_size_t(512)
    t = ft()
    assert fold(n, l, None, len(key_blob), b1, len(b1), b2, len(b2), out, C.byref(room), t.p) == _ffi.LH_ERR_ARG
    assert fold(n, l, cm, len(key_blob), None, len(b1), b2, len(b2), out, C.byref(room), t.p) == _ffi.LH_ERR_ARG
    assert fold(n, l, cm, len(key_blob), b1, len(b1), None, len(b2), out, C.byref(room), t.p) == _ffi.LH_ERR_ARG
    assert fold(n, l, cm, len(key_blob), b1, len(b1), b2, len(b2), None, C.byref(room), t.p) == _ffi.LH_ERR_ARG
    assert fold(n, l, cm, len(key_blob), b1, len(b1), b2, len(b2), out, None, t.p) == _ffi.LH_ERR_ARG
    assert fold(n, l, cm, len(key_blob), b1, len(b1), b2, len(b2), out, C.byref(room), None) == _ffi.LH_ERR_ARG
    short = C.c_size_t(160 + 32 * p - 1)
    assert fold(n, l, cm, len(key_blob), b1, len(b1), b2, len(b2), out, C.byref(short), t.p) == _ffi.LH_ERR_ARG
    assert b"LH_NOVA_INSTANCE_BYTES" in lib.lh_last_error()
    # a blob that cannot be read is the verifier's to refuse, whatever the room
    assert fold(n, l, cm, len(key_blob), b1, len(b1) - 1, b2, len(b2), out, C.byref(short), t.p) == _ffi.LH_ERR_INVALID_SNARK
    assert fold(n, 1, cm, len(key_blob), b1, len(b1), b2, len(b2), out, C.byref(room), t.p) == _ffi.LH_ERR_ARG
    assert b"dim_vars" in lib.lh_last_error()
    assert t.remaining() == len(rec["proof"]), "refused before a byte is read"
    # LH_NOVA_INSTANCE_BYTES(p) of room is what every fold takes: the last of the chain, whose first input is itself folded
    # (both points: the blob is that long already), with exactly that much; one byte less is refused
    last = [r for r in records if r["step"] == "fold"][-1]
    r1, r2 = arr(every[last["a"]]), arr(every[last["b"]])
    exact = 160 + 32 * p
    assert len(r1) == exact and hl.nova_instance_bytes(p) == exact
    out2, room2 = (C.c_uint8 * exact)(), C.c_size_t(exact)
    lt = hl.Keccak256Transcript.from_proof(last["proof"])
    assert fold(n, l, cm, len(key_blob), r1, len(r1), r2, len(r2), out2, C.byref(room2), lt.p) == _ffi.LH_OK
    assert bytes(out2[:room2.value]) == last["blob"] and room2.value == exact and not lt.remaining()
    room2 = C.c_size_t(exact - 1)
    lt = hl.Keccak256Transcript.from_proof(last["proof"])
    assert fold(n, l, cm, len(key_blob), r1, len(r1), r2, len(r2), out2, C.byref(room2), lt.p) == _ffi.LH_ERR_ARG
    assert lt.remaining() == len(last["proof"])
    # the prover's entries as far as they get without a device: the NULL ctx; never a crash on NULLs
    assert lib.lh_nova_instance(None, None, None, None, None, p, out, C.byref(room)) == _ffi.LH_ERR_ARG
    assert lib.lh_nova_fold(None, None, None, b1, len(b1), b2, len(b2), None, None, None, None, None, None, out, C.byref(room), t.p) == _ffi.LH_ERR_ARG
    assert lib.lh_spartan_prove_relaxed(None, None, None, ib, len(blob), None, None, t.p) == _ffi.LH_ERR_ARG
    assert lib.lh_debug_nova_spmv2(None, None, 0, None, None, None, None) == _ffi.LH_ERR_ARG
    assert lib.lh_debug_nova_cross_term(None, l, None, None, None, None, None, None, None, None) == _ffi.LH_ERR_ARG
    assert lib.lh_debug_nova_fold(None, l, None, None, None, None, None, None, None, None) == _ffi.LH_ERR_ARG
    for call_ in (lambda: hl.nova_instance(None, None, None, 1, [1]), lambda: hl.nova_fold(None, None, None, blob, 1, None, blob, 1, None, 1, 1),
                  lambda: hl.spartan_prove_relaxed(None, None, None, blob, 1, None), lambda: hl.nova_spmv2(None, None, 0, [1], [1])):
        with pytest.raises(hl.ArgumentError, match="freed"):  # no key
            call_()
