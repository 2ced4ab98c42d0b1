"""GPU: the Brakedown PCS (pcs/multilinear/brakedown.rs) against the Python restatement (tests/brakedown_ref.py) byte for
byte - encoded rows, root, proof - in the shape of the reference's PCS tests (pcs/multilinear.rs:293-406
run_commit_open_verify / run_batch_commit_open_verify), then through the host verifier; one large commitment against
the library's host encoder, and a change to a committed row caught by the verifier."""
import ctypes as C
import random

import numpy as np
import pytest

import brakedown_ref as br
from oracle.pyref.poly import evaluate

pytestmark = pytest.mark.gpu
P = br.P
SEED = bytes(range(7, 39))


def _first_column(hl, proof, pp):
    """the first opened column: replay the transcript up to its squeeze"""
    t = hl.Keccak256Transcript.from_proof(proof)
    if pp.num_rows > 1:
        t.squeeze_challenges(pp.num_rows)
        t.read_field_elements(pp.row_len * pp.num_proximity_testing)
    t.read_field_elements(pp.row_len)
    return (t.squeeze_challenge() & 0xFFFFFFFF) % pp.codeword_len


@pytest.mark.parametrize("spec,nv", [(6, nv) for nv in range(3, 13)] + [(1, 4), (1, 12)])
def test_brakedown_commit_open_verify(hl, ctx, spec, nv):
    rng = random.Random(100 * spec + nv)
    op = br.Params(nv, spec, SEED)
    pp, _ = hl.Brakedown.trim(hl.Brakedown.setup(ctx, nv, spec, SEED), 1 << nv)
    vp = hl.BrakedownVerifierParam.setup(nv, spec, SEED)
    assert pp.info() == op.info() == vp.info()
    with pytest.raises(hl.InvalidPcsParam):
        hl.Brakedown.trim(pp, 1 << (nv + 1))
    evals = [rng.randrange(P) for _ in range(1 << nv)]
    poly = hl.MultilinearPolynomial.new(ctx, evals)
    o_comm = br.commit(op, evals)
    comm = hl.Brakedown.commit(pp, poly)
    assert comm.rows(pp.num_rows, pp.codeword_len) == [x for row in o_comm.rows for x in row]
    assert comm.root == o_comm.root
    point = [rng.randrange(P) for _ in range(nv)]
    value = evaluate(evals, point)
    ot, t = br.Transcript(), hl.Keccak256Transcript()
    br.open_(op, evals, o_comm, point, ot)
    hl.Brakedown.open(pp, poly, comm, point, t)
    proof = t.into_proof()
    assert proof == ot.into_proof()
    for param in (vp, pp):
        r = hl.Keccak256Transcript.from_proof(proof)
        hl.Brakedown.verify(param, comm.root, point, value, r)
        assert r.remaining() == 0
    with pytest.raises(hl.InvalidPcsOpen, match="Consistency failure"):
        hl.Brakedown.verify(vp, comm.root, point, (value + 1) % P, hl.Keccak256Transcript.from_proof(proof))


def test_brakedown_batch_commit_open_verify(hl, ctx):
    nv, batch, spec = 6, 3, 6
    rng = random.Random(77)
    op = br.Params(nv, spec, SEED)
    pp, vp = hl.Brakedown.trim(hl.Brakedown.setup(ctx, nv, spec, SEED), 1 << nv)
    tables = [[rng.randrange(P) for _ in range(1 << nv)] for _ in range(batch)]
    polys = [hl.MultilinearPolynomial.new(ctx, tb) for tb in tables]
    ot, t = br.Transcript(), hl.Keccak256Transcript()
    o_comms = [br.commit(op, tb) for tb in tables]
    for c in o_comms:
        ot.write_hash(c.root)
    comms = hl.Brakedown.batch_commit_and_write(pp, polys, t)
    assert [c.root for c in comms] == [c.root for c in o_comms]
    pts = [t.squeeze_challenges(nv) for _ in range(2)]
    assert pts == [ot.squeeze_challenges(nv) for _ in range(2)]
    pairs = [(p, q) for p in range(batch) for q in range(2) if (p + q) % 3 != 2]
    vals = [evaluate(tables[p], pts[q]) for p, q in pairs]
    ot.write_field_elements(vals), t.write_field_elements(vals)
    for (p, q) in pairs:  # batch_open is one open per evaluation (brakedown.rs:278-300)
        br.open_(op, tables[p], o_comms[p], pts[q], ot)
    hl.Brakedown.batch_open(pp, nv, polys, comms, pts, [hl.Evaluation(p, q, v) for (p, q), v in zip(pairs, vals)], t)
    proof = t.into_proof()
    assert proof == ot.into_proof()
    r = hl.Keccak256Transcript.from_proof(proof)
    roots = hl.Brakedown.read_commitments(vp, batch, r)
    assert roots == [c.root for c in comms]
    assert r.squeeze_challenges(nv) == pts[0] and r.squeeze_challenges(nv) == pts[1]
    assert r.read_field_elements(len(vals)) == vals
    hl.Brakedown.batch_verify(vp, nv, roots, pts, [hl.Evaluation(p, q, v) for (p, q), v in zip(pairs, vals)], r)
    assert r.remaining() == 0


# (an ordinary GPU test, ~5 s: the suite's heavy-test estimates already fill LH_TEST_EST_LIMIT_S in tests/conftest.py)
def test_brakedown_2_22_rows_match_host_encoder_and_tamper_is_caught(hl, ctx):
    from halo2_lasso_amd import _ffi
    nv, spec = 22, 6
    pp = hl.Brakedown.setup(ctx, nv, spec, SEED)
    R, n, cw = pp.num_rows, pp.row_len, pp.codeword_len
    assert R > 1 and len(br.Params(nv, spec).a_dims) > 3  # several rows, several cascade levels
    # canonical limbs below r (top limb < r's) serve as Montgomery forms of field elements
    limbs = np.random.default_rng(22).integers(0, 1 << 63, size=(1 << nv, 4), dtype=np.uint64)
    limbs[:, 3] %= np.uint64(0x30644E72E131A029)
    raw = limbs.astype("<u8").tobytes()
    poly = hl.MultilinearPolynomial(ctx, ctx.upload(raw), nv)
    comm = hl.Brakedown.commit(pp, poly)
    rows = C.create_string_buffer(32 * R * cw)
    assert ctx.lib.lh_brakedown_comm_rows(ctx.h, comm.h, rows) == 0
    rows = rows.raw
    msg, out = (_ffi.lh_fr * n)(), (_ffi.lh_fr * cw)()
    for r in range(R):
        C.memmove(msg, raw[32 * n * r:32 * n * (r + 1)], 32 * n)
        assert ctx.lib.lh_brakedown_encode(pp.h, msg, out) == 0
        assert C.string_at(out, 32 * cw) == rows[32 * cw * r:32 * cw * (r + 1)], "row %d" % r
    rng = random.Random(5)
    point = [rng.randrange(P) for _ in range(nv)]
    value = hl.evaluate_polys(ctx, [poly], point)[0]
    t = hl.Keccak256Transcript()
    hl.Brakedown.open(pp, poly, comm, point, t)
    proof = t.into_proof()
    hl.Brakedown.verify(pp, comm.root, point, value, hl.Keccak256Transcript.from_proof(proof))
    # one bit of one committed entry, in the column the opening reads first (its index depends only on the rows written
    # before it, which come from the polynomial, not from the commitment)
    col, row = _first_column(hl, proof, pp), 3
    at = comm.rows_device_ptr() + 32 * (row * cw + col)
    entry = bytearray(_download(ctx, at))
    entry[0] ^= 1
    assert ctx.lib.lh_upload(ctx.h, at, bytes(entry), 32) == 0
    t = hl.Keccak256Transcript()
    hl.Brakedown.open(pp, poly, comm, point, t)
    with pytest.raises(hl.InvalidPcsOpen, match="^(Invalid merkle tree opening|Proximity failure)$"):
        hl.Brakedown.verify(pp, comm.root, point, value, hl.Keccak256Transcript.from_proof(t.into_proof()))


def _download(ctx, ptr):
    out = C.create_string_buffer(32)
    assert ctx.lib.lh_download(ctx.h, out, ptr, 32) == 0
    return out.raw
