"""CPU: batched Spartan, specification and host verifier (lh_spartan_verify_batch; the library has no device prover for it
yet: DESIGN.md section 27) - the specification (tests/spartan_batch_ref.py) against its golden file
(tests/golden/spartan_batch.json, tests/golden/make_spartan_batch.py: the six-variable cases are pinned there by length and
SHA-256, made here once by the specification and shared) and against the dense statement; the host verifier on those bytes, on
the cheating prover's and on damaged ones; the refusals that need no device; the exported symbols."""
import ctypes as C
import hashlib
import json
import os
import re

import pytest

import logup_gkr_ref as lgr
import spark_ref as spr
import spartan_batch_ref as sbr
import spartan_ref as spa
from oracle.pyref import kzg as o_kzg, sum_check as o_sc
from oracle.pyref.field import R_MOD as P
from oracle.pyref.transcript import Keccak256Transcript as OT, TranscriptError

HERE = os.path.dirname(os.path.abspath(__file__))
FILE = json.load(open(os.path.join(HERE, "golden", "spartan_batch.json")))
GOLDEN, FORGED = FILE["cases"], FILE["forgeries"]
SS = [int(x, 16) for x in json.load(open(os.path.join(HERE, "golden", "lasso_tables.json")))["srs"]["ss"]]
CASES = list(sbr.CASES)
PROVED = [c for c in CASES if c not in sbr.REFUSED]


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
        _MADE["key", case] = spa.commit(_pp(), sbr.case_instance(case)[0], sbr.CASES[case][1])
    return _MADE["key", case]


def _is(rec, prefix, data):
    return (len(data), hashlib.sha256(data).hexdigest()) == (rec[prefix + "bytes"], rec[prefix + "sha256"])


def golden(case):
    """-> (key blob, xs, proof): stored in full (`mid`) or made by the specification, once, and equal to the file in length
    and digest.  A case of spartan_batch_ref.REFUSED: the bytes written before the refusal."""
    if ("golden", case) in _MADE:
        return _MADE["golden", case]
    g = GOLDEN[case]
    _, ws, xs = sbr.case_instance(case)
    if case in sbr.SMALL:
        key = _key(case)
        t = OT()
        if case in sbr.REFUSED:
            with pytest.raises(TranscriptError, match=sbr.REFUSED[case]):
                sbr.prove(_pp(), key, ws, xs, t)
        else:
            sbr.prove(_pp(), key, ws, xs, t)
        key_blob, proof = key.blob, t.into_proof()
    else:
        key_blob, proof = bytes.fromhex(g["key"]), bytes.fromhex(g["proof"])
    assert _is(g, "key_", key_blob), "%s: the golden key is not what the specification produces now" % case
    assert _is(g, "", proof), "%s: the golden proof is not what the specification produces now" % case
    assert g["xs"] == [["%x" % v for v in x] for x in xs]
    _MADE["golden", case] = key_blob, xs, proof
    return _MADE["golden", case]


def forged(name):
    """-> (case, key blob, the public inputs the verifier is given, the proof) of a forgery, by the specification"""
    if ("forged", name) not in _MADE:
        case, ws, xs, xs_verified, forge = sbr.forgery(name)
        key = _key("four")  # (`three` is `four`'s first three instances over the same circuit: one key)
        t = OT()
        sbr.prove(_pp(), key, ws, xs, t, forge=forge)
        proof = t.into_proof()
        g = FORGED[name]
        assert g["case"] == case and _is(g, "", proof), "%s: the golden forgery is not what the specification produces now" % name
        assert g["xs"] == [["%x" % v for v in x] for x in xs_verified]
        _MADE["forged", name] = case, key.blob, xs_verified, proof
    return _MADE["forged", name]


def verify(hl, vp, case, **over):
    n, l, p, _ = sbr.CASES[case]
    key_blob, xs, proof = golden(case)
    a = dict(n=n, l=l, commitment=key_blob, xs=xs, proof=proof)
    a.update(over)
    hl.spartan_verify_batch(vp, a["n"], a["l"], a["commitment"], a["xs"], a["proof"])


# ------------------------------------------------------------------ 1. the specification
def test_the_cases_are_the_named_ones():
    assert set(GOLDEN) == set(sbr.CASES) and len(sbr.CASES) == 8 and set(FORGED) == set(sbr.FORGERIES)
    assert sbr.CASES == {"pair": (1, 2, 1, 2), "four": (3, 3, 2, 4), "three": (3, 3, 2, 3), "eight": (5, 3, 2, 8), "tall": (2, 4, 3, 4),
                         "full_public": (3, 3, 4, 2), "twice": (3, 3, 2, 2), "mid": (12, 10, 5, 5)}
    assert set(sbr.FORGERIES) == {"bad_witness", "bad_eval", "bad_public", "swapped_publics", "other_count"}
    assert {f: FORGED[f]["case"] for f in FORGED} == {"bad_witness": "four", "bad_eval": "four", "bad_public": "four",
                                                      "swapped_publics": "four", "other_count": "three"}
    assert sbr.SMALL == [c for c in CASES if c != "mid"] and len(SS) == 6 and sbr.MAX_BATCH_VARS == 26
    for case in CASES:
        n, l, p, count = sbr.CASES[case]
        g = GOLDEN[case]
        assert (g["n"], g["l"], g["p"], g["count"]) == (n, l, p, count) and len(g["xs"]) == count
    assert [c for c in CASES if "key" in GOLDEN[c] or "proof" in GOLDEN[c]] == ["mid"]
    # the one case the PCS refuses: the same assignment twice leaves a zero quotient, which no transcript writes
    assert list(sbr.REFUSED) == ["twice"] and [c for c in CASES if "error" in GOLDEN[c]] == ["twice"]
    # k + l - 1 of mid is 12; three and mid have zero instances; eight has k = 3
    n, l, p, count = sbr.CASES["mid"]
    assert sbr.batch_vars(count) + l - 1 == 12 and sbr.batch_vars(3) == 2 and sbr.batch_vars(8) == 3 and sbr.batch_vars(2) == 1
    assert sbr.case_instance("three")[1] == sbr.case_instance("four")[1][:3]
    assert sbr.case_instance("twice")[1][0] == sbr.case_instance("twice")[1][1]


@pytest.mark.parametrize("case", sbr.SMALL)
def test_reference_reproduces_the_golden(pp, case):
    n, l, p, count = sbr.CASES[case]
    inst, ws, xs = sbr.case_instance(case)
    key_blob, _, proof = golden(case)  # (made by the specification: length and digest are the file's)
    assert sbr.satisfied(inst, ws, xs, l) == (0, None), "every instance satisfies the dense statement"
    assert all(x[0] == 1 for x in xs)
    if case != "twice":
        assert len({tuple(w) for w in ws}) == count, "different assignments"
    k, K = sbr.batch_vars(count), 1 << sbr.batch_vars(count)
    Z = sbr.assignment(l, ws, xs)
    assert len(Z) == K << l and all(Z[i + K * y] == spa.assignment(l, ws[i], xs[i])[y] for i in range(count) for y in range(1 << l))
    assert all(Z[i + K * y] == 0 for i in range(count, K) for y in range(1 << l)), "the instances beyond K' are zero"
    if case in sbr.REFUSED:
        return
    sbr.verify(pp, n, l, key_blob, xs, OT(proof))
    # the layout: the W block, k + l outer rounds of 4, three values, l inner rounds of 3, four values
    assert int.from_bytes(proof[:32], "big") == 0 and len(proof) > 96 + 32 * (4 * (k + l) + 3 + 3 * l + 4)


def test_an_unsatisfying_batch_is_refused_by_the_specification(pp):
    inst, ws, xs = sbr.case_instance("four")
    key = _key("four")
    _, bad_ws, _, _, _ = sbr.forgery("bad_witness")
    assert sbr.satisfied(inst, bad_ws, xs, 3) == (1, 3), "one row of the LAST instance"
    t = OT()
    with pytest.raises(spa.SpartanError, match=r"the batch does not satisfy 1 of its constraints \(first: instance 3\)"):
        sbr.prove(pp, key, bad_ws, xs, t)
    assert t.into_proof() == b""
    other = [list(x) for x in xs]
    other[1][1] = (other[1][1] + 1) % P
    count, first = sbr.satisfied(inst, ws, other, 3)
    assert count >= 1 and first == 1
    with pytest.raises(spa.SpartanError, match=r"does not satisfy %d of its constraints \(first: instance 1\)" % count):
        sbr.prove(pp, key, ws, other, OT())
    for bad in (dict(ws=ws[:1], xs=xs[:1]), dict(ws=ws, xs=xs[:3])):
        with pytest.raises(spa.SpartanError):
            sbr.prove(pp, key, bad["ws"], bad["xs"], OT())


@pytest.mark.parametrize("name", list(sbr.FORGERIES))
def test_reference_refuses_the_forgeries(pp, name):
    case, key_blob, xs_verified, proof = forged(name)
    n, l, p, _ = sbr.CASES[case]
    with pytest.raises(spa.SpartanError, match=sbr.FORGERIES[name]):
        sbr.verify(pp, n, l, key_blob, xs_verified, OT(proof))
    honest = golden(case)
    if name in ("bad_public", "swapped_publics", "other_count"):  # the honest proof against other public inputs
        assert proof == honest[2] and xs_verified != honest[1]
    else:
        assert proof != honest[2] and xs_verified == honest[1]


# ------------------------------------------------------------------ 2. the host verifier
@pytest.mark.parametrize("case", PROVED)
def test_host_verifier_accepts_golden(hl, vp, vp_mid, case):
    verify(hl, vp if case in sbr.SMALL else vp_mid, case)


@pytest.mark.parametrize("name", list(sbr.FORGERIES))
def test_host_verifier_refuses_the_forgeries(hl, vp, name):
    case, key_blob, xs_verified, proof = forged(name)
    n, l, p, _ = sbr.CASES[case]
    with pytest.raises(hl.InvalidSnark, match="spartan: .*" + sbr.FORGERIES[name]):
        hl.spartan_verify_batch(vp, n, l, key_blob, xs_verified, proof)


def _sections(pp, case, monkeypatch):
    """where the sections of a golden proof begin: the specification's verifier is asked, at the entry of its pieces"""
    at = {}

    def spy(name, fn, tr_arg):
        def wrapped(*a, **k):
            at.setdefault(name, []).append(a[tr_arg].pos)
            return fn(*a, **k)
        return wrapped

    monkeypatch.setattr(o_sc, "verify", spy("sum-check", o_sc.verify, 4))
    monkeypatch.setattr(o_kzg, "batch_verify", spy("opening", o_kzg.batch_verify, 5))
    monkeypatch.setattr(spr, "verify", spy("spark", spr.verify, 7))
    n, l, p, _ = sbr.CASES[case]
    key_blob, xs, proof = golden(case)
    sbr.verify(pp, n, l, key_blob, xs, OT(proof))
    monkeypatch.undo()
    return at


@pytest.mark.parametrize("case", ["four", "three", "tall"])
def test_a_flipped_byte_in_each_section_is_invalid_snark(hl, vp, pp, monkeypatch, case):
    n, l, p, count = sbr.CASES[case]
    k = sbr.batch_vars(count)
    key_blob, xs, proof = golden(case)
    at = _sections(pp, case, monkeypatch)
    outer, inner = at["sum-check"][0], at["sum-check"][1]
    opens, sparks = at["opening"], at["spark"]
    assert outer == 96 and inner == outer + 32 * (4 * (k + l) + 3) and opens[0] == inner + 32 * (3 * l + 4) and len(sparks) == 3
    assert len([o for o in opens if o < sparks[0]]) == 1, "ONE opening of the stacked witness"
    where = {"W mask": 31, "W point": 40, "W point y": 90, "outer rounds": outer + 3, "outer last round": inner - 32 * 3 - 5,
             "vA": inner - 32 * 3 + 1, "vB": inner - 32 * 2 + 9, "vC": inner - 2, "inner rounds": inner + 7,
             "inner last round": opens[0] - 32 * 4 - 3, "eA": opens[0] - 32 * 4 + 3, "eB": opens[0] - 32 * 3 + 3, "eC": opens[0] - 32 - 4,
             "e_w": opens[0] - 3, "opening of W": opens[0] + 9, "last quotient before Spark": sparks[0] - 6, "Spark A": sparks[0] + 40,
             "Spark B": sparks[1] + 40, "Spark C": sparks[2] + 40, "last quotient": len(proof) - 7}
    for name, pos in where.items():
        bad = bytearray(proof)
        bad[pos] ^= 4
        with pytest.raises(hl.InvalidSnark, match="spartan: "):
            verify(hl, vp, case, proof=bytes(bad))
            pytest.fail("a flipped byte in the %s section verified" % name)
    # every public input of every instance, and each part of the key
    for i in range(count):
        for j in range(p):
            other = [list(x) for x in xs]
            other[i][j] = (other[i][j] + 1) % P
            with pytest.raises(hl.InvalidSnark, match="spartan: "):
                verify(hl, vp, case, xs=other)
    start = 0
    for b in spa.split_key(key_blob):
        for pos in (start + 31, start + 32 + 3, start + len(b) - 2):
            bad = bytearray(key_blob)
            bad[pos] ^= 4
            with pytest.raises(hl.InvalidSnark, match="spartan: "):
                verify(hl, vp, case, commitment=bytes(bad))
        start += len(b)


def test_other_inputs_lengths_and_shapes_are_invalid_snark(hl, vp):
    case = "four"
    n, l, p, count = sbr.CASES[case]
    key_blob, xs, proof = golden(case)
    verify(hl, vp, case)
    # another p: one element more or less per instance; another K': an instance more (another k too) or less (the same k)
    for other in ([x + [0] for x in xs], [x[:1] for x in xs], xs + [[0] * p], xs[:3], xs[:2], xs + [[1] + [0] * (p - 1)] * 4):
        with pytest.raises(hl.InvalidSnark, match="spartan: "):
            verify(hl, vp, case, xs=other)
    # three's proof with a zero fourth instance said aloud: K' is absorbed (the forgery other_count), and four's as three
    with pytest.raises(hl.InvalidSnark, match="spartan: "):
        hl.spartan_verify_batch(vp, n, l, key_blob, golden("three")[1] + [[0] * p], golden("three")[2])
    # another key
    with pytest.raises(hl.InvalidSnark):
        verify(hl, vp, case, commitment=golden("full_public")[0])
    with pytest.raises(hl.InvalidSnark, match="spartan: trailing bytes"):
        verify(hl, vp, case, proof=proof + b"\0")
    for cut in (proof[:-1], proof[:2000], proof[:700], proof[:95], proof[:40], b""):  # a proof that ends early
        with pytest.raises(hl.InvalidSnark):
            verify(hl, vp, case, proof=cut)
    with pytest.raises(hl.InvalidSnark, match="spartan: "):  # a W mask out of range
        verify(hl, vp, case, proof=b"\0" * 31 + b"\x02" + proof[32:])
    parts = spa.split_key(key_blob)
    for bad in (key_blob[:-1], key_blob + b"\0", parts[0] + parts[1], b"\0" * 31 + b"\x80" + key_blob[32:], b""):
        with pytest.raises(hl.InvalidSnark, match="spartan: malformed"):
            verify(hl, vp, case, commitment=bad)
    for other in (dict(n=n - 1), dict(n=n + 1), dict(l=l + 1), dict(l=l - 1, xs=[x[:1] + x[1:2] for x in xs])):
        with pytest.raises(hl.InvalidSnark):  # another shape
            verify(hl, vp, case, **other)


def test_plain_and_batch_proofs_are_not_each_others(hl, vp):
    """a plain lh_spartan_verify refuses a batch proof, and the batch verifier a plain one - over one key and public input"""
    n, l, p, _ = sbr.CASES["four"]
    key_blob, xs, proof = golden("four")
    with pytest.raises(hl.InvalidSnark, match="spartan: "):
        hl.spartan_verify(vp, n, l, key_blob, xs[0], proof)
    inst, ws, _ = sbr.case_instance("four")
    t = OT()
    spa.prove(_pp(), _key("four"), ws[0], xs[0], t)
    plain = t.into_proof()
    hl.spartan_verify(vp, n, l, key_blob, xs[0], plain)
    with pytest.raises(hl.InvalidSnark, match="spartan: "):
        hl.spartan_verify_batch(vp, n, l, key_blob, [xs[0], xs[0]], plain)
    with pytest.raises(hl.InvalidSnark, match="spartan: "):
        hl.spartan_verify_batch(vp, n, l, key_blob, xs, plain)


# ------------------------------------------------------------------ 3. refusals that need no device, the exported symbols
def test_argument_refusals_and_symbols(hl, vp):
    from halo2_lasso_amd import _ffi
    lib = _ffi.load()
    root = os.path.dirname(HERE)
    header = open(os.path.join(root, "include", "lasso_hip.h")).read()
    rust = open(os.path.join(root, "bindings", "rust", "src", "sys.rs")).read()
    for sym in ("lh_spartan_verify_batch",):
        assert hasattr(lib, sym) and sym in _ffi.SIGNATURES and re.search(r"lh_status %s\(" % sym, header), sym
        assert re.search(r"pub fn %s\(" % sym, rust), sym
    assert "#define LH_SPARTAN_BATCH_MAX_VARS 26\n" in header and _ffi.LH_SPARTAN_BATCH_MAX_VARS == 26
    assert "pub const LH_SPARTAN_BATCH_MAX_VARS: usize = 26;" in rust
    assert callable(hl.spartan_verify_batch)
    makefile = open(os.path.join(root, "halo2-lasso_amd", "csrc", "Makefile")).read()
    assert " spartan_batch.o" in makefile

    case = "four"
    n, l, p, count = sbr.CASES[case]
    key_blob, xs, proof = golden(case)
    for bad in (dict(n=0), dict(n=31), dict(l=1, xs=[x[:1] for x in xs]), dict(l=25), dict(xs=[[] for _ in xs]), dict(xs=[x + [0] * 3 for x in xs]),
                dict(xs=xs[:1]), dict(xs=[]), dict(xs=[xs[0], xs[1][:1]]), dict(commitment=None), dict(proof=None), dict(xs=None)):
        with pytest.raises(hl.ArgumentError):
            verify(hl, vp, case, **bad)
    with pytest.raises(hl.ArgumentError, match="batch_vars"):  # 24 + 3 variables
        verify(hl, vp, case, l=24, xs=[xs[0]] * 5)
    with pytest.raises(hl.InvalidPcsParam):
        verify(hl, vp, case, n=7)
    with pytest.raises(hl.InvalidPcsParam):  # k + l - 1 = 7 over an SRS of six
        verify(hl, vp, case, l=6)
    with pytest.raises(hl.InvalidPcsParam):  # k = 5: 5 + 3 - 1 = 7
        verify(hl, vp, case, xs=[xs[0]] * 17)
    # the same through ctypes: the library's own answers
    flat = [v for x in xs for v in x]
    arr = lambda b: (C.c_uint8 * len(b)).from_buffer_copy(b)
    cm, xa = arr(key_blob), hl._fr_array(flat)
    tr = lambda: hl.Keccak256Transcript.from_proof(proof)
    t = tr()
    call = lib.lh_spartan_verify_batch
    assert call(vp.h, n, l, cm, len(key_blob), xa, count, p, tr().p) == _ffi.LH_OK
    assert call(None, n, l, cm, len(key_blob), xa, count, p, t.p) == _ffi.LH_ERR_ARG
    assert call(vp.h, n, l, None, len(key_blob), xa, count, p, t.p) == _ffi.LH_ERR_ARG
    assert call(vp.h, n, l, cm, len(key_blob), None, count, p, t.p) == _ffi.LH_ERR_ARG
    assert call(vp.h, n, l, cm, len(key_blob), xa, count, p, None) == _ffi.LH_ERR_ARG
    for bn, bl, bc, bp, word in ((0, l, count, p, b"num_vars"), (31, l, count, p, b"num_vars"), (n, 1, count, 1, b"dim_vars"),
                                 (n, 25, count, p, b"dim_vars"), (n, l, count, 0, b"num_public"), (n, l, count, 5, b"num_public"),
                                 (n, l, 1, p, b"num_instances"), (n, l, 0, p, b"num_instances"), (n, 24, 5, p, b"batch_vars"),
                                 (n, l, 1 << 40, p, b"batch_vars")):
        assert call(vp.h, bn, bl, cm, len(key_blob), xa, bc, bp, t.p) == _ffi.LH_ERR_ARG, (bn, bl, bc, bp)
        assert word in lib.lh_last_error()
    assert call(vp.h, 7, l, cm, len(key_blob), xa, count, p, t.p) == _ffi.LH_ERR_INVALID_PCS_PARAM
    assert call(vp.h, n, 6, cm, len(key_blob), xa, count, p, t.p) == _ffi.LH_ERR_INVALID_PCS_PARAM
    assert call(vp.h, n, l, cm, len(key_blob) - 1, xa, count, p, t.p) == _ffi.LH_ERR_INVALID_SNARK
    assert b"spartan: malformed" in lib.lh_last_error()
    assert t.remaining() == len(proof), "refused before a byte is read"
