"""Ligero PCS, host side (no GPU): the specification (tests/ligero_ref.py) against direct evaluation, the library's
parameters and host encoder against the specification, the restated commit, open and verify against brakedown_ref's own with
its encoder swapped, the C++ verifier on the specification's proofs (tests/golden/ligero.json: accepted, and refused with the
reference's strings when forged, truncated or made under the other code), the argument refusals and the new symbols."""
import ctypes as C
import hashlib
import json
import os
import random

import pytest

import brakedown_ref as br
import ligero_ref as lr
from oracle.pyref.poly import evaluate

P = lr.P
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "ligero.json")) as _f:
    FIXTURE = json.load(_f)
_proofs = {}


def _golden(case):
    if case not in _proofs:
        _proofs[case] = lr.golden_proof(case)
    return _proofs[case]


# ------------------------------------------------------------------ parameters
def test_roots_of_unity_have_their_order():
    assert pow(lr.ROOT_2_28, 1 << 28, P) == 1 and pow(lr.ROOT_2_28, 1 << 27, P) == P - 1
    assert (P - 1) % (1 << 28) == 0 and (P - 1) % (1 << 29) != 0
    for k in (0, 1, 5, 28):
        w = lr.root_of_unity(k)
        assert pow(w, 1 << k, P) == 1 and (k == 0 or pow(w, 1 << (k - 1), P) == P - 1)
    assert lr.root_of_unity(5) == pow(lr.root_of_unity(7), 4, P)


def test_column_counts_and_chosen_rows():
    assert [lr.num_column_opening(b) for b in (1, 2, 3)] == [487, 309, 258]
    assert {lr.num_proximity_testing(n) for n in range(1, 29)} == {1}
    want = list(range(1, 9)) + [8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13, 14, 14, 15, 15, 16, 16, 17]
    for b in (1, 2, 3):
        assert [lr.choose_row_vars(nv, b) for nv in range(1, 27)] == want


@pytest.mark.parametrize("b", [1, 2, 3])
def test_param_info_matches_the_specification(hl, b):
    for nv in range(1, 27):
        vp = hl.LigeroVerifierParam.derive(nv, b)
        assert vp.info() == lr.Params(nv, b).info(), nv
        assert (vp.log_inv_rate, vp.row_vars, vp.suffix) == (b, lr.choose_row_vars(nv, b), "_brakedown")
    for rv in range(7):
        assert hl.LigeroVerifierParam.derive(6, b, rv).info() == lr.Params(6, b, rv).info(), rv
    assert isinstance(hl.LigeroVerifierParam.derive(6, b), hl.BrakedownParam)


def test_argument_refusals(hl):
    from halo2_lasso_amd import _ffi
    lib, AUTO, ARG = _ffi.load(), _ffi.LH_LIGERO_ROW_VARS_AUTO, _ffi.LH_ERR_ARG
    for args in [(6, 0), (6, 4), (0, 2), (27, 2), (6, 2, 7), (26, 3, 26)]:
        with pytest.raises(hl.ArgumentError):
            hl.LigeroVerifierParam.derive(*args)
        with pytest.raises(hl.ArgumentError):
            hl.LigeroVerifierParam.setup(*args)
        with pytest.raises(hl.ArgumentError):
            hl.Ligero.setup(None, *args)
    with pytest.raises(hl.ArgumentError):
        hl.LigeroVerifierParam.derive(6, 2, -1)
    out = C.c_void_p()
    bad = [lib.lh_ligero_derive(6, 0, AUTO, C.byref(out)), lib.lh_ligero_derive(6, 4, AUTO, C.byref(out)),
           lib.lh_ligero_derive(0, 2, AUTO, C.byref(out)), lib.lh_ligero_derive(27, 2, AUTO, C.byref(out)),
           lib.lh_ligero_derive(6, 2, 7, C.byref(out)), lib.lh_ligero_derive(26, 3, 26, C.byref(out)),
           lib.lh_ligero_derive(6, 2, AUTO, None), lib.lh_ligero_setup(None, 6, 2, AUTO, None),
           lib.lh_ligero_setup(None, 6, 5, AUTO, C.byref(out)), lib.lh_ligero_setup(None, 6, 2, 7, C.byref(out))]
    assert bad == [ARG] * len(bad) and not out.value
    # row_vars + log_inv_rate = 28 is the last that exists
    assert hl.LigeroVerifierParam.derive(26, 2, 26).info()[2] == 1 << 28
    # parameters alone cannot encode; trim is to the setup size only
    vp = hl.LigeroVerifierParam.derive(3, 2)
    cw = (_ffi.lh_fr * vp.codeword_len)()
    assert lib.lh_brakedown_encode(vp.h, cw, cw) == ARG
    assert hl.Brakedown.trim(vp, 8) == (vp, vp)
    with pytest.raises(hl.InvalidPcsParam):
        hl.Brakedown.trim(vp, 16)


# ------------------------------------------------------------------ the code
@pytest.mark.parametrize("b", [1, 2, 3])
@pytest.mark.parametrize("row_vars", range(5))
def test_codeword_is_the_interpolated_polynomial_on_the_stated_points(row_vars, b):
    rng = random.Random(10 * row_vars + b)
    pp = lr.Params(max(row_vars, 1), b, row_vars)
    K, N = pp.row_len, pp.codeword_len
    msg = [rng.randrange(P) for _ in range(K)]
    cw = lr.encode(pp, msg)
    assert len(cw) == N and cw[:K] == msg
    f = lr.interpolate(msg)
    w_n, w_k = lr.root_of_unity(pp.depth), lr.root_of_unity(row_vars)
    for i in range(1 << b):
        for j in range(K):
            assert cw[i * K + j] == br._horner(f, pow(w_n, i, P) * pow(w_k, j, P) % P), (i, j)
    # linear
    msg2 = [rng.randrange(P) for _ in range(K)]
    c = rng.randrange(P)
    assert lr.encode(pp, [(x + c * y) % P for x, y in zip(msg, msg2)]) == \
        [(x + c * y) % P for x, y in zip(cw, lr.encode(pp, msg2))]
    # MDS: a non-zero polynomial of degree < K has at most K - 1 roots among the N points
    for at in {0, K // 2, K - 1}:
        unit = [0] * K
        unit[at] = 1
        assert sum(1 for x in lr.encode(pp, unit) if x) >= N - K + 1
    if K == 1:
        assert cw == msg * N


@pytest.mark.parametrize("b", [1, 2])
@pytest.mark.parametrize("row_vars", range(14))
def test_host_encoder_matches_the_specification(hl, row_vars, b):
    nv = max(row_vars, 1)
    vp = hl.LigeroVerifierParam.setup(nv, b, row_vars)
    op = lr.Params(nv, b, row_vars)
    assert vp.info() == op.info()
    rng = random.Random(100 * row_vars + b)
    msg = [rng.randrange(P) for _ in range(op.row_len)]
    assert vp.encode(msg) == lr.encode(op, msg)


def test_host_encoder_at_rate_one_eighth(hl):
    vp, op = hl.LigeroVerifierParam.setup(5, 3, 4), lr.Params(5, 3, 4)
    msg = list(range(1, 17))
    assert vp.encode(msg) == lr.encode(op, msg)


# ------------------------------------------------------------------ the scheme is brakedown_ref's
@pytest.mark.parametrize("case", [(4, 2, None), (6, 1, 4)])
def test_restated_scheme_is_brakedown_refs_with_the_encoder_swapped(monkeypatch, case):
    pp, root, point, value, proof = _golden(case) if case in lr.GOLDEN_CASES else lr.golden_proof(case)
    rng = random.Random("ligero %d %d %r" % case)
    evals = [rng.randrange(P) for _ in range(1 << case[0])]
    monkeypatch.setattr(br, "encode", lr.encode)
    comm = br.commit(pp, evals)
    mine = lr.commit(pp, evals)
    assert comm.rows == mine.rows and comm.hashes == mine.hashes and comm.root == root
    tr = br.Transcript()
    br.open_(pp, evals, comm, point, tr)
    assert tr.into_proof() == proof
    br.verify(pp, root, point, value, br.Transcript(proof))
    lr.verify(pp, root, point, value, lr.Transcript(proof))
    for verify in (br.verify, lr.verify):
        with pytest.raises(br.PcsError, match="Consistency failure"):
            verify(pp, root, point, (value + 1) % P, br.Transcript(proof))
        bad = bytearray(proof)
        bad[31] ^= 1
        with pytest.raises(br.PcsError, match="Proximity failure"):
            verify(pp, root, point, value, br.Transcript(bytes(bad)))


# ------------------------------------------------------------------ the host verifier
def test_golden_set_is_what_the_fixture_says():
    assert sorted(FIXTURE) == sorted(lr.golden_name(c) for c in lr.GOLDEN_CASES)
    assert {FIXTURE[lr.golden_name(c)]["info"][1] for c in lr.GOLDEN_CASES} >= {1, 2, 4, 64}
    assert "proof_file" in FIXTURE[lr.golden_name(lr.GOLDEN_FULL)]


@pytest.mark.parametrize("case", lr.GOLDEN_CASES, ids=lr.golden_name)
def test_host_verifier_accepts_golden_proofs(hl, case):
    fx = FIXTURE[lr.golden_name(case)]
    if "proof_file" in fx:  # stored whole: nothing of the specification runs
        root, value = bytes.fromhex(fx["root"]), int(fx["value"], 16)
        with open(os.path.join(ROOT, "tests", "golden", fx["proof_file"]), "rb") as f:
            proof = f.read()
        point = [int(x, 16) for x in fx["point"]]
    else:
        pp, root, point, value, proof = _golden(case)
        assert list(pp.info()) == fx["info"] and pp.depth == fx["depth"]
    assert root.hex() == fx["root"] and "%064x" % value == fx["value"]
    assert len(proof) == fx["proof_len"] and hashlib.sha256(proof).hexdigest() == fx["proof_sha256"]
    K, R, N, t, ldt = fx["info"]
    assert len(proof) == 32 * ((1 + ldt) * K * (R > 1) + K * (R == 1) + t * (R + fx["depth"]))
    vp = hl.LigeroVerifierParam.setup(*case)
    r = hl.Keccak256Transcript.from_proof(proof)
    hl.Brakedown.verify(vp, root, point, value, r)
    assert r.remaining() == 0


@pytest.mark.parametrize("case", [(6, 2, None), (6, 2, 5)], ids=lr.golden_name)
def test_host_verifier_refuses_forgeries(hl, case):
    pp, root, point, value, proof = _golden(case)
    vp = hl.LigeroVerifierParam.setup(*case)
    K, R = pp.row_len, pp.num_rows
    rows = (2 * K if R > 1 else K)
    t0_row = 32 * (rows - K)             # the t_0 row is the last row written
    column = 32 * rows                   # the first opened column's entries, then its path
    path = column + 32 * R

    def check(data, message, val=value, rt=root):
        with pytest.raises(hl.InvalidPcsOpen, match="^%s$" % message):
            hl.Brakedown.verify(vp, rt, point, val, hl.Keccak256Transcript.from_proof(bytes(data)))

    def flipped(at):
        b = bytearray(proof)
        b[at] ^= 1
        return b
    if R > 1:
        check(flipped(31), "Proximity failure")              # the proximity row
    check(flipped(t0_row + 31), "Proximity failure")         # the t_0 row
    check(flipped(column + 31), "(Proximity failure|Invalid merkle tree opening)")  # a column entry
    check(flipped(path + 5), "Invalid merkle tree opening")  # a path node
    check(proof, "Consistency failure", val=(value + 1) % P)
    check(proof, "Invalid merkle tree opening", rt=bytes([root[0] ^ 1]) + root[1:])
    for cut in (0, 31, t0_row + 32, len(proof) - 1):
        with pytest.raises(hl.Error):
            hl.Brakedown.verify(vp, root, point, value, hl.Keccak256Transcript.from_proof(proof[:cut]))
    hl.Brakedown.verify(vp, root, point, value, hl.Keccak256Transcript.from_proof(proof))


def test_a_proof_under_the_other_code_is_refused(hl):
    nv, seed = 6, bytes(range(32))
    lig = hl.LigeroVerifierParam.setup(nv, 2)
    bd = hl.BrakedownVerifierParam.setup(nv, 6, seed)
    assert lig.info()[:2] == bd.info()[:2] == (64, 1)  # the same rows, another code
    _, root, point, value, proof = _golden((nv, 2, None))
    with pytest.raises(hl.Error):
        hl.Brakedown.verify(bd, root, point, value, hl.Keccak256Transcript.from_proof(proof))
    op = br.Params(nv, 6, seed)
    rng = random.Random(8)
    evals = [rng.randrange(P) for _ in range(1 << nv)]
    comm = br.commit(op, evals)
    tr = br.Transcript()
    br.open_(op, evals, comm, point, tr)
    bd_proof = tr.into_proof()
    hl.Brakedown.verify(bd, comm.root, point, evaluate(evals, point), hl.Keccak256Transcript.from_proof(bd_proof))
    with pytest.raises(hl.Error):
        hl.Brakedown.verify(lig, comm.root, point, evaluate(evals, point), hl.Keccak256Transcript.from_proof(bd_proof))


# ------------------------------------------------------------------ the new symbols, in every layer
def test_new_symbols_are_declared_everywhere():
    from halo2_lasso_amd import _ffi
    lib = _ffi.load()
    header = open(os.path.join(ROOT, "include", "lasso_hip.h")).read()
    sys_rs = open(os.path.join(ROOT, "bindings", "rust", "src", "sys.rs")).read()
    for name in ("lh_ligero_setup", "lh_ligero_derive"):
        assert getattr(lib, name) is not None
        assert name in _ffi.SIGNATURES
        assert "lh_status %s(" % name in header
        assert "pub fn %s(" % name in sys_rs
    assert "#define LH_LIGERO_ROW_VARS_AUTO ((size_t)-1)" in header
    assert _ffi.LH_LIGERO_ROW_VARS_AUTO == C.c_size_t(-1).value
