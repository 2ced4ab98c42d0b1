"""Brakedown PCS, host side (no GPU): the parameters against the reference's own table and the Python restatement
(tests/brakedown_ref.py), the host-only setup and encoder, the C++ verifier on proofs the oracle made (accepted, and
rejected with the reference's error strings when tampered with), the hash half of the transcript, NULL arguments."""
import ctypes as C
import random

import pytest

import brakedown_ref as br
from oracle.pyref.keccak import keccak_f
from oracle.pyref.poly import evaluate

P = br.P
SEED = bytes(range(32))


# code/brakedown.rs:372-390: (delta, c_n, d_n, num_column_opening) and num_proximity_testing at log2_q 127 / 254
REFERENCE_TABLE = {
    1: (0.02, 6, 33, 13265, 2, 1),
    2: (0.03, 7, 26, 8768, 2, 1),
    3: (0.04, 7, 22, 6593, 2, 1),
    4: (0.05, 8, 19, 5279, 2, 1),
    5: (0.06, 9, 21, 4390, 2, 1),
    6: (0.07, 10, 20, 3755, 2, 1),
}


@pytest.mark.parametrize("spec", range(1, 7))
def test_python_spec_reproduces_reference_table(spec):
    s, n, n_0 = br.Spec(spec), 1 << 30, 30
    delta, c_n, d_n, nco, npt_127, npt_254 = REFERENCE_TABLE[spec]
    assert s.delta() - delta < 1e-3
    assert s.c_n(n) == c_n
    assert s.d_n(127, n) == d_n and s.d_n(254, n) == d_n
    assert s.num_column_opening() == nco
    assert s.num_proximity_testing(127, n, n_0) == npt_127
    assert s.num_proximity_testing(254, n, n_0) == npt_254


def test_fast_keccak_is_the_oracle_permutation():
    rng = random.Random(3)
    for _ in range(4):
        st = [rng.getrandbits(64) for _ in range(25)]
        assert br.keccak_f_fast(st) == keccak_f(st)


@pytest.mark.parametrize("spec", range(1, 7))
def test_param_info_matches_python(hl, spec):
    for nv in range(1, 27):
        try:
            want = br.Params(nv, spec).info()
        except br.PcsError:
            want = None  # the reference's dimensions underflow (a panic there)
        if want is None:
            with pytest.raises(hl.ArgumentError):
                hl.BrakedownVerifierParam.derive(nv, spec)
            continue
        assert hl.BrakedownVerifierParam.derive(nv, spec).info() == want, (spec, nv)


@pytest.mark.parametrize("nv,spec", [(4, 6), (7, 1), (9, 3), (11, 6)])
def test_host_setup_and_encoder_match_python(hl, nv, spec):
    vp = hl.BrakedownVerifierParam.setup(nv, spec, SEED)
    op = br.Params(nv, spec, SEED)
    assert vp.info() == op.info()
    rng = random.Random(nv)
    msg = [rng.randrange(P) for _ in range(op.row_len)]
    assert vp.encode(msg) == br.encode(op, msg)
    # encoding is linear
    msg2 = [rng.randrange(P) for _ in range(op.row_len)]
    s = [(x + y) % P for x, y in zip(msg, msg2)]
    assert vp.encode(s) == [(x + y) % P for x, y in zip(vp.encode(msg), vp.encode(msg2))]


def test_trim_only_to_the_setup_size(hl):
    vp = hl.BrakedownVerifierParam.derive(6, 6)
    assert hl.Brakedown.trim(vp, 64) == (vp, vp)
    with pytest.raises(hl.InvalidPcsParam, match="Can't trim MultilinearBrakedownParams into different poly_size"):
        hl.Brakedown.trim(vp, 32)


def _oracle_proof(nv, spec, seed=SEED, rng_seed=0):
    op = br.Params(nv, spec, seed)
    rng = random.Random(1000 * nv + spec + rng_seed)
    evals = [rng.randrange(P) for _ in range(1 << nv)]
    comm = br.commit(op, evals)
    point = [rng.randrange(P) for _ in range(nv)]
    tr = br.Transcript()
    br.open_(op, evals, comm, point, tr)
    return op, comm.root, point, evaluate(evals, point), tr.into_proof()


@pytest.mark.parametrize("nv", range(3, 11))
def test_host_verifier_accepts_oracle_proofs(hl, nv):
    op, root, point, value, proof = _oracle_proof(nv, 6)
    vp = hl.BrakedownVerifierParam.setup(nv, 6, SEED)
    t = hl.Keccak256Transcript.from_proof(proof)
    hl.Brakedown.verify(vp, root, point, value, t)
    assert t.remaining() == 0


def test_host_verifier_accepts_spec1(hl):
    op, root, point, value, proof = _oracle_proof(5, 1)
    hl.Brakedown.verify(hl.BrakedownVerifierParam.setup(5, 1, SEED), root, point, value,
                        hl.Keccak256Transcript.from_proof(proof))


def test_host_verifier_rejects_tampered_proofs(hl):
    nv = 6
    op, root, point, value, proof = _oracle_proof(nv, 6)
    vp = hl.BrakedownVerifierParam.setup(nv, 6, SEED)
    assert op.num_rows == 1
    first_column = 32 * op.row_len  # the t_0 row (the polynomial itself), then column 0's entries
    first_sibling = first_column + 32 * op.num_rows

    def flipped(at):
        b = bytearray(proof)
        b[at] ^= 1  # the low bit of a big-endian field element / of a hash byte
        return bytes(b)

    with pytest.raises(hl.InvalidPcsOpen, match="^Proximity failure$"):
        hl.Brakedown.verify(vp, root, point, value, hl.Keccak256Transcript.from_proof(flipped(first_sibling - 1)))
    with pytest.raises(hl.InvalidPcsOpen, match="^Invalid merkle tree opening$"):
        hl.Brakedown.verify(vp, root, point, value, hl.Keccak256Transcript.from_proof(flipped(first_sibling + 5)))
    with pytest.raises(hl.InvalidPcsOpen, match="^Consistency failure$"):
        hl.Brakedown.verify(vp, root, point, (value + 1) % P, hl.Keccak256Transcript.from_proof(proof))
    other = hl.BrakedownVerifierParam.setup(nv, 6, bytes(32))  # other matrices: the rows no longer encode
    with pytest.raises(hl.InvalidPcsOpen, match="^Proximity failure$"):
        hl.Brakedown.verify(other, root, point, value, hl.Keccak256Transcript.from_proof(proof))


def test_hash_transcript_writes_raw_bytes_and_absorbs_nothing(hl):
    h = bytes(range(100, 132))
    t, u = hl.Keccak256Transcript(), hl.Keccak256Transcript()
    t.write_field_element(5), u.write_field_element(5)
    t.write_hash(h)
    assert t.squeeze_challenge() == u.squeeze_challenge()
    proof = t.into_proof()
    assert proof[32:] == h
    ot = br.Transcript()
    ot.write_field_element(5)
    ot.write_hash(h)
    assert ot.into_proof() == proof
    r = hl.Keccak256Transcript.from_proof(proof)
    assert r.read_field_element() == 5 and r.read_hash() == h
    with pytest.raises(hl.TranscriptError):
        r.read_hash()
    assert hl.Brakedown.read_commitments(hl.BrakedownVerifierParam.derive(3, 6), 1,
                                         hl.Keccak256Transcript.from_proof(h)) == [h]


def test_null_arguments_are_errors(hl):
    from halo2_lasso_amd import _ffi
    lib = _ffi.load()
    ARG = _ffi.LH_ERR_ARG
    vp = hl.BrakedownVerifierParam.setup(3, 6, SEED)
    tr = hl.Keccak256Transcript()
    hio = tr.hash_io()
    sz = [C.c_size_t() for _ in range(5)]
    out = C.c_void_p()
    fr3 = (_ffi.lh_fr * 3)()
    cw = (_ffi.lh_fr * vp.codeword_len)()
    bad = [
        lib.lh_keccak_transcript_hash_io(None, C.byref(_ffi.lh_hash_transcript())),
        lib.lh_keccak_transcript_hash_io(tr.p, None),
        lib.lh_brakedown_setup(None, 3, 6, None, C.byref(out)),
        lib.lh_brakedown_setup(None, 3, 6, SEED, None),
        lib.lh_brakedown_derive(3, 6, None),
        lib.lh_brakedown_param_info(None, *[C.byref(x) for x in sz]),
        lib.lh_brakedown_param_info(vp.h, None, *[C.byref(x) for x in sz[1:]]),
        lib.lh_brakedown_trim(None, 8),
        lib.lh_brakedown_encode(None, cw, cw),
        lib.lh_brakedown_encode(vp.h, None, cw),
        lib.lh_brakedown_encode(vp.h, cw, None),
        lib.lh_brakedown_commit(None, vp.h, None, 3, C.byref(out)),
        lib.lh_brakedown_batch_commit(None, vp.h, None, 1, 3, C.byref(out)),
        lib.lh_brakedown_comm_root(None, C.create_string_buffer(32)),
        lib.lh_brakedown_comm_rows(None, None, None),
        lib.lh_brakedown_comm_rows_device(None, C.byref(out)),
        lib.lh_brakedown_open(None, vp.h, None, 3, None, fr3, tr.p, C.byref(hio)),
        lib.lh_brakedown_batch_open(None, vp.h, 3, None, None, 0, None, 0, None, 0, tr.p, C.byref(hio)),
        lib.lh_brakedown_read_commitments(None, 1, C.byref(hio), C.create_string_buffer(32)),
        lib.lh_brakedown_read_commitments(vp.h, 1, None, C.create_string_buffer(32)),
        lib.lh_brakedown_read_commitments(vp.h, 1, C.byref(hio), None),
        lib.lh_brakedown_verify(None, bytes(32), fr3, 3, fr3, tr.p, C.byref(hio)),
        lib.lh_brakedown_verify(vp.h, None, fr3, 3, fr3, tr.p, C.byref(hio)),
        lib.lh_brakedown_verify(vp.h, bytes(32), None, 3, fr3, tr.p, C.byref(hio)),
        lib.lh_brakedown_verify(vp.h, bytes(32), fr3, 3, None, tr.p, C.byref(hio)),
        lib.lh_brakedown_verify(vp.h, bytes(32), fr3, 3, fr3, None, C.byref(hio)),
        lib.lh_brakedown_verify(vp.h, bytes(32), fr3, 3, fr3, tr.p, None),
        lib.lh_brakedown_batch_verify(None, 3, bytes(32), 1, fr3, 1, (_ffi.lh_evaluation * 1)(), 1, tr.p,
                                      C.byref(hio)),
        lib.lh_brakedown_batch_verify(vp.h, 3, None, 1, fr3, 1, (_ffi.lh_evaluation * 1)(), 1, tr.p, C.byref(hio)),
        lib.lh_brakedown_batch_verify(vp.h, 3, bytes(32), 1, None, 1, (_ffi.lh_evaluation * 1)(), 1, tr.p,
                                      C.byref(hio)),
        lib.lh_brakedown_batch_verify(vp.h, 3, bytes(32), 1, fr3, 1, None, 1, tr.p, C.byref(hio)),
    ]
    assert bad == [ARG] * len(bad), bad
    # a param without matrices cannot encode
    assert lib.lh_brakedown_encode(hl.BrakedownVerifierParam.derive(3, 6).h, cw, cw) == ARG
