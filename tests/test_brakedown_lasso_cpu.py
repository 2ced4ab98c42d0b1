"""CPU: Lasso over MultilinearBrakedown without a device - the oracle glue of tests/brakedown_lasso_ref.py against the fixture,
and the library's host verifier (lh_lasso_verify_brakedown) on the oracle's proof of case (c): accepted as it is, rejected
with a bit flipped in a root, in the mask element or in a written evaluation, under another num_vars, and with a byte
appended.  The oracle's own verify takes over a minute per proof and is not run."""
import ctypes as C
import hashlib

import pytest

import brakedown_lasso_ref as bl
import brakedown_ref as br

CASE = "c"


@pytest.fixture(scope="module")
def proved():
    """-> (proof, roots, number of evaluations) of case (c) by the oracle, made once (~7 s)"""
    return bl.oracle_prove(CASE)


def _table(hl):
    kind, c, l, n, _ = bl.CASES[CASE]
    assert kind == "xor"
    return hl.LassoTable.bitwise(hl.SUBTABLE_XOR, c, l), c, l, n


def _open_bytes(p):
    rows = (p.num_proximity_testing + 1) * p.row_len if p.num_rows > 1 else p.row_len
    return 32 * (rows + p.num_column_opening * (p.num_rows + p.depth))


def test_glue_reproduces_the_fixture(proved):
    proof, roots, num_evals = proved
    fx = bl.fixture()[CASE]
    kind, c, l, n, _ = bl.CASES[CASE]
    assert fx["case"] == [kind, c, l, n] and fx["num_vars"] == max(n, l)
    assert num_evals == fx["num_evaluations"] == 1 + 3 * c + 2 * c
    assert len(proof) == fx["proof_len"]
    assert hashlib.sha256(proof).hexdigest() == fx["proof_sha256"]
    assert [r.hex() for r in roots] == fx["roots"]
    # the framing: the mask element (zero), then the roots as raw bytes
    assert proof[:32] == bytes(32)
    assert proof[32:32 + 32 * len(roots)] == b"".join(roots)
    # read_ts is identically zero (pairwise distinct indices) and still has a root of its own, the zero column's
    zero_root = br.commit(br.Params(max(n, l), bl.SPEC, bl.SEED), [0] * (1 << max(n, l))).root
    assert roots[1 + c] == zero_root


def test_host_verifier_accepts_the_oracles_proof_and_rejects_changes(hl, proved):
    proof, roots, num_evals = proved
    table, c, l, n = _table(hl)
    nv = max(n, l)
    vp = hl.BrakedownVerifierParam.setup(nv, bl.SPEC, bl.SEED)
    r = hl.Keccak256Transcript.from_proof(proof)
    hl.lasso_verify(vp, table, n, r)
    assert r.remaining() == 0

    def verify(data, param=vp, num_vars=n):
        hl.lasso_verify(param, table, num_vars, hl.Keccak256Transcript.from_proof(bytes(data)))

    bad = bytearray(proof)
    bad[32 + 5] ^= 1  # the root of a
    with pytest.raises(hl.InvalidPcsOpen, match="^Invalid merkle tree opening$"):
        verify(bad)
    bad = bytearray(proof)
    bad[32 + 32 * (len(roots) - 1) + 31] ^= 0x80  # the last root, final_cts_0
    with pytest.raises(hl.InvalidPcsOpen, match="^Invalid merkle tree opening$"):
        verify(bad)
    bad = bytearray(proof)
    bad[31] ^= 1  # the mask element (field elements travel most significant byte first): "commitment 0 is the identity"
    with pytest.raises(hl.InvalidSnark, match="mask out of range"):
        verify(bad)
    # the proof ends in the 3 c + alpha evaluations at r_N / r_M and one opening per evaluation
    p = br.Params(nv, bl.SPEC)
    evals_at = len(proof) - num_evals * _open_bytes(p) - 32 * (3 * c + c)
    assert evals_at > 32 + 32 * len(roots)
    bad = bytearray(proof)
    bad[evals_at + 31] ^= 1  # dim_0(r_N)
    with pytest.raises(hl.InvalidSnark):
        verify(bad)
    with pytest.raises(hl.InvalidPcsParam, match="param supports %d variates but got %d" % (nv + 1, nv)):
        verify(proof, param=hl.BrakedownVerifierParam.setup(nv + 1, bl.SPEC, bl.SEED))
    with pytest.raises(hl.Error):
        verify(proof, num_vars=n + 1)  # (max(n + 1, l) is still the param's size: the argument itself fails)
    with pytest.raises(hl.InvalidSnark, match="trailing bytes"):
        verify(proof + b"\x00")
    # ... at the boundary itself, not only in the Python wrapper
    r = hl.Keccak256Transcript.from_proof(proof + b"\x00")
    t = table.to_c()
    rc = vp.lib.lh_lasso_verify_brakedown(vp.h, C.byref(t), n, r.p, C.byref(r.hash_io()))
    assert rc == hl._ffi.LH_ERR_INVALID_SNARK and b"trailing bytes" in vp.lib.lh_last_error()


def test_null_arguments(hl):
    from halo2_lasso_amd import _ffi
    table, c, l, n = _table(hl)
    vp = hl.BrakedownVerifierParam.derive(max(n, l), bl.SPEC)
    lib, t = vp.lib, table.to_c()
    tr = hl.Keccak256Transcript()
    hio = C.byref(tr.hash_io())
    dims = (C.c_void_p * 1)(None)
    bad = [lib.lh_lasso_verify_brakedown(None, C.byref(t), n, tr.p, hio),
           lib.lh_lasso_verify_brakedown(vp.h, None, n, tr.p, hio),
           lib.lh_lasso_verify_brakedown(vp.h, C.byref(t), n, None, hio),
           lib.lh_lasso_verify_brakedown(vp.h, C.byref(t), n, tr.p, None),
           lib.lh_lasso_prove_brakedown(None, vp.h, C.byref(t), n, dims, tr.p, hio),
           lib.lh_brakedown_commit_columns(None, vp.h, dims, (C.c_int * 1)(1), (C.c_size_t * 1)(0), 1, (C.c_void_p * 1)())]
    assert bad == [_ffi.LH_ERR_ARG] * len(bad), bad
    assert tr.into_proof() == b""
