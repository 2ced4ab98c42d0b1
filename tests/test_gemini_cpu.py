"""CPU: Gemini over univariate KZG and the batched univariate KZG opening under it - the Python restatement
(tests/gemini_ref.py) on itself, and the library's host verifiers (lh_ukzg_* / lh_gemini_* verify entries, no GPU) on the
restatement's proofs.

The shapes follow pcs/multilinear.rs run_commit_open_verify / run_batch_commit_open_verify and the tests at the end of
pcs/univariate/kzg.rs (from line 577).  One-variable openings and the all-zero table end in the reference with a
TranscriptError (the identity commitment cannot be written, util/transcript.rs:172-179; gemini_ref's docstring): they are
tested as that error, here for the restatement and in test_gpu_gemini.py for the library.

tests/golden/gemini_vectors.json was written once by `python tests/test_gemini_cpu.py` (the __main__ block below).
"""
import ctypes as C
import json
import os
import random

import pytest

if __name__ == "__main__":  # (under pytest tests/conftest.py has done this)
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gemini_ref as gr
from oracle.pyref import curve, zeromorph as o_zm
from oracle.pyref.field import R_MOD as P, Q_MOD
from oracle.pyref.poly import evaluate
from oracle.pyref.transcript import Keccak256Transcript as OT, TranscriptError

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemini_vectors.json")


# ------------------------------------------------------------------ proofs by the restatement
def gemini_proof(n, seed, extra=0, table=None):
    """run_commit_open_verify (pcs/multilinear.rs): commitment, point squeezed, evaluation written, opening"""
    rng = random.Random(seed)
    s = rng.randrange(1, P)
    pp, vp = gr.trim(gr.setup(s, (1 << n) + extra), 1 << n)
    table = [rng.randrange(P) for _ in range(1 << n)] if table is None else table
    t = OT()
    comm = gr.batch_commit_and_write(pp, [table], t)[0]
    point = t.squeeze_challenges(n)
    ev = evaluate(table, point)
    t.write_field_element(ev)
    gr.open_(pp, table, point, ev, t)
    return dict(s=s, n=n, table=table, comm=comm, point=point, eval=ev, proof=t.into_proof()), vp


def gemini_check(vp, n, proof, verify, from_proof):
    t = from_proof(proof)
    comm = t.read_commitments(1)[0]
    point = t.squeeze_challenges(n)
    ev = t.read_field_element()
    verify(vp, comm, point, ev, t)
    return t


def gemini_batch_proof(n, batch, seed):
    """run_batch_commit_open_verify: `batch` polys, batch points, evaluations that repeat points and polys"""
    rng = random.Random(seed)
    s = rng.randrange(1, P)
    pp, vp = gr.trim(gr.setup(s, 1 << n), 1 << n)
    polys = [[rng.randrange(P) for _ in range(1 << n)] for _ in range(batch)]
    queries = _queries(batch, batch, rng)
    t = OT()
    gr.batch_commit_and_write(pp, polys, t)
    points = [t.squeeze_challenges(n) for _ in range(batch)]
    evals = [gr.Evaluation(i, j, evaluate(polys[i], points[j])) for i, j in queries]
    t.write_field_elements([e.value for e in evals])
    gr.batch_open(pp, n, polys, points, evals, t)
    return dict(s=s, n=n, batch=batch, polys=polys, queries=queries, proof=t.into_proof()), vp


def _queries(num_polys, num_points, rng):
    """kzg.rs:626-633: every point on poly 0, every poly on point 0, then random pairs; unique, in order"""
    qs = [(0, j) for j in range(num_points)] + [(i, 0) for i in range(1, num_polys)]
    qs += [(rng.randrange(num_polys), rng.randrange(num_points)) for _ in range(num_polys)]
    return list(dict.fromkeys(qs))


def gemini_batch_check(vp, n, batch, queries, proof, batch_verify, from_proof, mk_eval):
    t = from_proof(proof)
    comms = t.read_commitments(batch)
    points = [t.squeeze_challenges(n) for _ in range(batch)]
    values = t.read_field_elements(len(queries))
    batch_verify(vp, n, comms, points, [mk_eval(i, j, v) for (i, j), v in zip(queries, values)], t)
    return t


def ukzg_batch_proof(lens, num_points, queries, seed, swap=None):
    """kzg.rs:613-655 with polys of the given lengths; queries = (poly, point) pairs as given (duplicates allowed)"""
    rng = random.Random(seed)
    s = rng.randrange(1, P)
    pp, vp = gr.trim(gr.setup(s, max(lens)), max(lens))
    polys = [[rng.randrange(P) for _ in range(m)] for m in lens]
    t = OT()
    t.write_commitments([gr.ukzg_commit(pp, p) for p in polys])
    points = t.squeeze_challenges(num_points)
    evals = [gr.Evaluation(i, j, gr.poly_eval(polys[i], points[j])) for i, j in queries]
    t.write_field_elements([e.value for e in evals])
    gr.ukzg_batch_open(pp, polys, points, evals, t)
    return dict(s=s, lens=lens, num_points=num_points, polys=polys, queries=queries, proof=t.into_proof()), vp


def ukzg_batch_check(vp, num_polys, num_points, queries, proof, batch_verify, from_proof, mk_eval):
    t = from_proof(proof)
    comms = t.read_commitments(num_polys)
    points = t.squeeze_challenges(num_points)
    values = t.read_field_elements(len(queries))
    batch_verify(vp, comms, points, [mk_eval(i, j, v) for (i, j), v in zip(queries, values)], t)
    return t


UKZG_SHAPES = {
    # polys of different lengths, shared point sets given in different order, a duplicated (poly, point) pair
    "mixed": ([8, 5, 8, 3, 1], 3, [(0, 0), (0, 1), (1, 1), (1, 0), (2, 2), (3, 0), (3, 0), (4, 1), (2, 0), (2, 1)]),
    "one_set": ([6, 6], 2, [(0, 0), (0, 1), (1, 1), (1, 0)]),
    "single": ([7], 1, [(0, 0)]),
    "kzg_rs": ([16] * 4, 2, [(0, 0), (0, 1), (1, 0), (2, 0), (3, 0), (2, 1), (1, 1)]),
}


def _tamperings(proof, value_offset):
    """a wrong evaluation (its low bit flipped), a flipped proof (one flipped bit would take the last commitment, the KZG
    proof pi, off the curve and end as a TranscriptError before any check: its sign is flipped instead, y -> q - y), a
    swapped commitment (the first commitment exchanged for another valid point, the generator)"""
    wrong_eval = bytearray(proof)
    wrong_eval[value_offset + 31] ^= 1
    flipped = bytearray(proof)
    flipped[-32:] = (Q_MOD - int.from_bytes(proof[-32:], "big")).to_bytes(32, "big")
    swapped = bytearray(proof)
    swapped[0:64] = (1).to_bytes(32, "big") + (2).to_bytes(32, "big")
    return {"wrong evaluation": bytes(wrong_eval), "flipped byte": bytes(flipped), "swapped commitment": bytes(swapped)}


# ------------------------------------------------------------------ the restatement on itself
@pytest.mark.parametrize("n", [2, 3, 4, 5, 6])
def test_oracle_gemini_commit_open_verify(n):
    d, vp = gemini_proof(n, 100 + n)
    assert len(d["proof"]) == 64 + 32 + 96 * n + 64
    assert d["comm"] == o_zm.commit_coeffs(gr.setup(d["s"], 1 << n).powers_g1, d["table"])
    t = gemini_check(vp, n, d["proof"], gr.verify, OT)
    assert t.pos == len(t.stream)
    for what, bad in _tamperings(d["proof"], 64).items():
        with pytest.raises((gr.PcsError, TranscriptError)):
            gemini_check(vp, n, bad, gr.verify, OT)


def test_oracle_gemini_one_variable_and_zero_table_end_as_the_reference_does():
    """gemini.rs:78-138 at n = 1: the only quotient fs[0] div (X^2 - beta^2) is zero, its commitment is the identity, and
    write_commitment refuses it (transcript.rs:172-179).  The all-zero table fails earlier, at the first fold commitment."""
    with pytest.raises(TranscriptError, match="Invalid elliptic curve point encoding"):
        gemini_proof(1, 101)
    rng = random.Random(5)
    pp, _ = gr.trim(gr.setup(rng.randrange(1, P), 8), 8)
    t = OT()
    with pytest.raises(TranscriptError, match="Invalid elliptic curve point encoding"):
        gr.open_(pp, [0] * 8, [3, 5, 7], 0, t)
    assert t.into_proof() == b""


def test_oracle_gemini_upper_half_zero():
    """leading zero coefficients are dropped by the reference's UnivariatePolynomial: same commitment, same proof shape"""
    n = 4
    rng = random.Random(77)
    d, vp = gemini_proof(n, 78, table=[rng.randrange(P) for _ in range(8)] + [0] * 8)
    assert len(d["proof"]) == 64 + 32 + 96 * n + 64
    gemini_check(vp, n, d["proof"], gr.verify, OT)


@pytest.mark.parametrize("n,batch", [(2, 2), (3, 4), (4, 3)])
def test_oracle_gemini_batch(n, batch):
    d, vp = gemini_batch_proof(n, batch, 200 + n)
    gemini_batch_check(vp, n, batch, d["queries"], d["proof"], gr.batch_verify, OT, gr.Evaluation)
    bad = bytearray(d["proof"])
    bad[64 * batch + 31] ^= 1  # the first evaluation
    with pytest.raises(Exception):
        gemini_batch_check(vp, n, batch, d["queries"], bytes(bad), gr.batch_verify, OT, gr.Evaluation)


@pytest.mark.parametrize("shape", sorted(UKZG_SHAPES))
def test_oracle_ukzg_batch(shape):
    lens, npts, queries = UKZG_SHAPES[shape]
    d, vp = ukzg_batch_proof(lens, npts, queries, 300 + len(lens))
    t = ukzg_batch_check(vp, len(lens), npts, queries, d["proof"], gr.ukzg_batch_verify, OT, gr.Evaluation)
    assert t.pos == len(t.stream)
    for what, bad in _tamperings(d["proof"], 64 * len(lens)).items():
        with pytest.raises((gr.PcsError, TranscriptError)):
            ukzg_batch_check(vp, len(lens), npts, queries, bad, gr.ukzg_batch_verify, OT, gr.Evaluation)


def test_oracle_ukzg_single_open():
    rng = random.Random(11)
    s = rng.randrange(1, P)
    pp, vp = gr.trim(gr.setup(s, 8), 8)
    poly = [rng.randrange(P) for _ in range(8)]
    t = OT()
    t.write_commitment(gr.ukzg_commit(pp, poly))
    x = t.squeeze_challenge()
    t.write_field_element(gr.poly_eval(poly, x))
    gr.ukzg_open(pp, poly, x, t)
    r = OT(t.into_proof())
    gr.ukzg_verify(vp, r.read_commitment(), r.squeeze_challenge(), r.read_field_element(), r)
    with pytest.raises(gr.PcsError, match="Too large degree of poly to commit"):
        gr.ukzg_commit(pp, poly + [1])
    assert gr.ukzg_commit(pp, poly + [0, 0]) == gr.ukzg_commit(pp, poly)  # leading zeros are dropped first


def test_division_is_schoolbook_and_agrees_with_successive_linear_factors():
    """the product's shortcut (factor by factor, remainders dropped) against the oracle's division, on the oracle's side"""
    rng = random.Random(3)
    f = [rng.randrange(P) for _ in range(13)]
    pts = [rng.randrange(P) for _ in range(3)]
    q, r = gr.div_rem(f, gr.vanishing_poly(pts))
    step = f
    for p in pts:
        step, _ = gr.div_rem(step, [(-p) % P, 1])
    assert q == step and len(r) <= 3
    z = rng.randrange(P)
    assert gr.poly_eval(f, z) == (gr.poly_eval(q, z) * gr.vanishing_eval(pts, z) + gr.poly_eval(r, z)) % P
    b = rng.randrange(P)
    q2, _ = gr.div_rem(f, [(-b * b) % P, 0, 1])
    assert q2 == gr.div_rem(f, gr.vanishing_poly([b, (-b) % P]))[0]
    assert gr.div_rem([1, 2], [5, 0, 1]) == ([], [1, 2])


# ------------------------------------------------------------------ eval_sets: fixed expected structure
def _sets(queries):
    sets, superset = gr.eval_sets([gr.Evaluation(i, j, 1000 * i + j) for i, j in queries])
    return [(s.polys, s.points, s.diffs, s.evals) for s in sets], superset


def test_eval_sets_gemini_shape():
    n = 4
    sets, superset = _sets([(0, 0), (0, 1)] + [(i, i + 1) for i in range(1, n)])
    assert superset == [0, 1, 2, 3, 4] and len(sets) == n
    assert sets[0] == ([0], [0, 1], [2, 3, 4], [[0, 1]])
    for i in range(1, n):
        assert sets[i] == ([i], [i + 1], [p for p in range(n + 1) if p != i + 1], [[1000 * i + i + 1]])


def test_eval_sets_shared_point_set_in_different_order():
    sets, superset = _sets([(0, 0), (0, 1), (1, 1), (1, 0), (2, 2)])
    assert superset == [0, 1, 2]
    # poly 1's evaluations are reordered to the set's point order
    assert sets == [([0, 1], [0, 1], [2], [[0, 1], [1000, 1001]]), ([2], [2], [0, 1], [[2002]])]


def test_eval_sets_duplicated_pair():
    sets, superset = _sets([(0, 0), (1, 0), (0, 0), (1, 0), (1, 1)])
    assert superset == [0, 1]
    assert sets == [([0], [0], [1], [[0]]), ([1], [0, 1], [], [[1000, 1001]])]


def test_eval_sets_one_set_only():
    sets, superset = _sets([(0, 0), (1, 0)])
    assert sets == [([0, 1], [0], [], [[0], [1000]])]
    scalars, normalizer = gr.set_scalars(gr.eval_sets([gr.Evaluation(0, 0, 1), gr.Evaluation(1, 0, 2)])[0], [1], [5], 9)
    assert (scalars, normalizer) == ([1], 1)  # the vanishing polynomial of an empty `diffs` is 1


# ------------------------------------------------------------------ the library's host verifiers on the restatement's proofs
def _lib_eval(hl):
    return lambda i, j, v: hl.Evaluation(i, j, v)


@pytest.mark.parametrize("n", [2, 3, 5])
def test_library_gemini_verifier_on_oracle_proofs(hl, n):
    """fails on the parent commit (no such symbol): the test this feature turns green without a GPU"""
    d, _ = gemini_proof(n, 100 + n)
    vp = hl.GeminiVerifierParam.setup(d["s"])
    t = gemini_check(vp, n, d["proof"], hl.Gemini.verify, hl.Keccak256Transcript.from_proof)
    assert t.remaining() == 0
    for what, bad in _tamperings(d["proof"], 64).items():
        with pytest.raises(hl.InvalidPcsOpen, match="Invalid univariate KZG open"):
            gemini_check(vp, n, bad, hl.Gemini.verify, hl.Keccak256Transcript.from_proof)


@pytest.mark.parametrize("n,batch", [(2, 2), (3, 4)])
def test_library_gemini_batch_verifier_on_oracle_proofs(hl, n, batch):
    d, _ = gemini_batch_proof(n, batch, 200 + n)
    vp = hl.GeminiVerifierParam.setup(d["s"])
    t = gemini_batch_check(vp, n, batch, d["queries"], d["proof"], hl.Gemini.batch_verify,
                           hl.Keccak256Transcript.from_proof, _lib_eval(hl))
    assert t.remaining() == 0
    bad = bytearray(d["proof"])
    bad[64 * batch + 31] ^= 1
    with pytest.raises(hl.Error):
        gemini_batch_check(vp, n, batch, d["queries"], bytes(bad), hl.Gemini.batch_verify,
                           hl.Keccak256Transcript.from_proof, _lib_eval(hl))


@pytest.mark.parametrize("shape", sorted(UKZG_SHAPES))
def test_library_ukzg_batch_verifier_on_oracle_proofs(hl, shape):
    lens, npts, queries = UKZG_SHAPES[shape]
    d, _ = ukzg_batch_proof(lens, npts, queries, 300 + len(lens))
    vp = hl.UnivariateKzgVerifierParam.setup(d["s"])
    t = ukzg_batch_check(vp, len(lens), npts, queries, d["proof"], hl.UnivariateKzg.batch_verify,
                         hl.Keccak256Transcript.from_proof, _lib_eval(hl))
    assert t.remaining() == 0
    for what, bad in _tamperings(d["proof"], 64 * len(lens)).items():
        with pytest.raises(hl.InvalidPcsOpen, match="Invalid univariate KZG open"):
            ukzg_batch_check(vp, len(lens), npts, queries, bad, hl.UnivariateKzg.batch_verify,
                             hl.Keccak256Transcript.from_proof, _lib_eval(hl))


def test_library_ukzg_single_verifier_and_param_round_trip(hl):
    from oracle.pyref import pairing
    rng = random.Random(11)
    s = rng.randrange(1, P)
    pp, _ = gr.trim(gr.setup(s, 8), 8)
    poly = [rng.randrange(P) for _ in range(8)]
    t = OT()
    t.write_commitment(gr.ukzg_commit(pp, poly))
    x = t.squeeze_challenge()
    t.write_field_element(gr.poly_eval(poly, x))
    gr.ukzg_open(pp, poly, x, t)
    vp = hl.UnivariateKzgVerifierParam.setup(s)
    g1, g2, s_g2 = vp.export()
    assert g1 == curve.G1_GEN and g2 == pairing.G2_GEN and s_g2 == pairing.g2_mul(pairing.G2_GEN, s)
    for v in (vp, hl.UnivariateKzgVerifierParam.new(g1, g2, s_g2)):
        r = hl.Keccak256Transcript.from_proof(t.into_proof())
        hl.UnivariateKzg.verify(v, r.read_commitment(), r.squeeze_challenge(), r.read_field_element(), r)
        r = hl.Keccak256Transcript.from_proof(t.into_proof())
        with pytest.raises(hl.InvalidPcsOpen, match="Invalid univariate KZG open"):
            hl.UnivariateKzg.verify(v, r.read_commitment(), r.squeeze_challenge(), (r.read_field_element() + 1) % P, r)


# ------------------------------------------------------------------ golden vectors
def _golden_cases():
    out = {"gemini": [], "ukzg_batch": []}
    for n in (2, 5):
        d, _ = gemini_proof(n, 7000 + n)
        out["gemini"].append(dict(n=n, s=hex(d["s"]), table=[hex(v) for v in d["table"]], point=[hex(v) for v in d["point"]],
                                  eval=hex(d["eval"]), proof=d["proof"].hex()))
    # n = 1: what the reference leaves in the transcript before write_commitment refuses the identity [q]
    rng = random.Random(7001)
    s = rng.randrange(1, P)
    pp, _ = gr.trim(gr.setup(s, 2), 2)
    table, t = [rng.randrange(P) for _ in range(2)], OT()
    gr.batch_commit_and_write(pp, [table], t)
    point = t.squeeze_challenges(1)
    t.write_field_element(evaluate(table, point))
    try:
        gr.open_(pp, table, point, 0, t)
        raise AssertionError("expected the identity commitment to be refused")
    except TranscriptError:
        pass
    out["gemini_one_variable"] = dict(n=1, s=hex(s), table=[hex(v) for v in table], point=[hex(v) for v in point],
                                      error="Invalid elliptic curve point encoding", written=t.into_proof().hex())
    lens, npts, queries = UKZG_SHAPES["mixed"]
    d, _ = ukzg_batch_proof(lens, npts, queries, 7100)
    out["ukzg_batch"].append(dict(s=hex(d["s"]), lens=lens, num_points=npts, queries=[list(q) for q in queries],
                                  polys=[[hex(v) for v in p] for p in d["polys"]], proof=d["proof"].hex()))
    return out


def test_golden_vectors_oracle_and_library(hl):
    """the recorded proofs still come out of the restatement, and both verifiers accept them: oracle and product cannot
    drift together unnoticed"""
    with open(GOLDEN) as f:
        gold = json.load(f)
    assert gold == _golden_cases()
    for g in gold["gemini"]:
        s, n, proof = int(g["s"], 16), g["n"], bytes.fromhex(g["proof"])
        gemini_check(gr.VerifierParam(s), n, proof, gr.verify, OT)
        t = gemini_check(hl.GeminiVerifierParam.setup(s), n, proof, hl.Gemini.verify, hl.Keccak256Transcript.from_proof)
        assert t.remaining() == 0 and t.squeeze_challenge() is not None
    g = gold["gemini_one_variable"]
    assert len(bytes.fromhex(g["written"])) == 64 + 32 + 32  # commitment, evaluation, fs[0](-beta); then the refused [q]
    for g in gold["ukzg_batch"]:
        s, proof, queries = int(g["s"], 16), bytes.fromhex(g["proof"]), [tuple(q) for q in g["queries"]]
        ukzg_batch_check(gr.VerifierParam(s), len(g["lens"]), g["num_points"], queries, proof, gr.ukzg_batch_verify, OT,
                         gr.Evaluation)
        ukzg_batch_check(hl.UnivariateKzgVerifierParam.setup(s), len(g["lens"]), g["num_points"], queries, proof,
                         hl.UnivariateKzg.batch_verify, hl.Keccak256Transcript.from_proof, _lib_eval(hl))


# ------------------------------------------------------------------ NULL arguments of the host-only entry points
def test_null_arguments_of_the_verifier_entry_points(hl):
    """every pointer goes through NEED / NEED_N (capi.cpp): NULL is LH_ERR_ARG, never a crash.  The entry points that take a
    ctx are covered on the GPU (test_gpu_gemini.py)."""
    from halo2_lasso_amd import _ffi
    lib = _ffi.load()
    vp = hl.GeminiVerifierParam.setup(5)
    tr = hl.Keccak256Transcript.from_proof(b"\0" * 256)
    g1, fr, g2, h = _ffi.lh_g1(), _ffi.lh_fr(), _ffi.lh_g2(), C.c_void_p()
    ev = (_ffi.lh_evaluation * 1)()
    tbl = hl.LassoTable.range(2, 4).to_c()
    bad = [
        lib.lh_ukzg_vp_setup(None, C.byref(h)), lib.lh_ukzg_vp_setup(C.byref(fr), None),
        lib.lh_ukzg_vp_new(None, C.byref(g2), C.byref(g2), C.byref(h)), lib.lh_ukzg_vp_new(C.byref(g1), None, C.byref(g2), C.byref(h)),
        lib.lh_ukzg_vp_new(C.byref(g1), C.byref(g2), None, C.byref(h)), lib.lh_ukzg_vp_new(C.byref(g1), C.byref(g2), C.byref(g2), None),
        lib.lh_ukzg_vp_export(None, C.byref(g1), C.byref(g2), C.byref(g2)), lib.lh_ukzg_vp_export(vp.h, None, C.byref(g2), C.byref(g2)),
        lib.lh_ukzg_vp_export(vp.h, C.byref(g1), None, C.byref(g2)), lib.lh_ukzg_vp_export(vp.h, C.byref(g1), C.byref(g2), None),
        lib.lh_ukzg_verify(None, C.byref(g1), C.byref(fr), C.byref(fr), tr.p), lib.lh_ukzg_verify(vp.h, None, C.byref(fr), C.byref(fr), tr.p),
        lib.lh_ukzg_verify(vp.h, C.byref(g1), None, C.byref(fr), tr.p), lib.lh_ukzg_verify(vp.h, C.byref(g1), C.byref(fr), None, tr.p),
        lib.lh_ukzg_verify(vp.h, C.byref(g1), C.byref(fr), C.byref(fr), None),
        lib.lh_ukzg_batch_verify(None, C.byref(g1), 1, C.byref(fr), 1, ev, 1, tr.p),
        lib.lh_ukzg_batch_verify(vp.h, None, 1, C.byref(fr), 1, ev, 1, tr.p),
        lib.lh_ukzg_batch_verify(vp.h, C.byref(g1), 1, None, 1, ev, 1, tr.p),
        lib.lh_ukzg_batch_verify(vp.h, C.byref(g1), 1, C.byref(fr), 1, None, 1, tr.p),
        lib.lh_ukzg_batch_verify(vp.h, C.byref(g1), 1, C.byref(fr), 1, ev, 1, None),
        lib.lh_gemini_verify(None, C.byref(g1), C.byref(fr), 1, C.byref(fr), tr.p),
        lib.lh_gemini_verify(vp.h, None, C.byref(fr), 1, C.byref(fr), tr.p),
        lib.lh_gemini_verify(vp.h, C.byref(g1), None, 1, C.byref(fr), tr.p),
        lib.lh_gemini_verify(vp.h, C.byref(g1), C.byref(fr), 1, None, tr.p),
        lib.lh_gemini_verify(vp.h, C.byref(g1), C.byref(fr), 1, C.byref(fr), None),
        lib.lh_gemini_batch_verify(None, 1, C.byref(g1), 1, C.byref(fr), 1, ev, 1, tr.p),
        lib.lh_gemini_batch_verify(vp.h, 1, None, 1, C.byref(fr), 1, ev, 1, tr.p),
        lib.lh_gemini_batch_verify(vp.h, 1, C.byref(g1), 1, None, 1, ev, 1, tr.p),
        lib.lh_gemini_batch_verify(vp.h, 1, C.byref(g1), 1, C.byref(fr), 1, None, 1, tr.p),
        lib.lh_gemini_batch_verify(vp.h, 1, C.byref(g1), 1, C.byref(fr), 1, ev, 1, None),
        lib.lh_lasso_verify_gemini(None, C.byref(tbl), 2, tr.p), lib.lh_lasso_verify_gemini(vp.h, None, 2, tr.p),
        lib.lh_lasso_verify_gemini(vp.h, C.byref(tbl), 2, None),
        lib.lh_hyperplonk_verify_gemini(None, None, None, tr.p), lib.lh_hyperplonk_verify_gemini(vp.h, None, None, tr.p),
        lib.lh_hyperplonk_verify_phases_gemini(None, None, 0, None, None, None, tr.p),
        lib.lh_hyperplonk_verify_phases_gemini(vp.h, None, 0, None, None, None, tr.p),
    ]
    assert bad == [_ffi.LH_ERR_ARG] * len(bad), bad
    lib.lh_ukzg_vp_free(None)


if __name__ == "__main__":
    with open(GOLDEN, "w") as f:
        json.dump(_golden_cases(), f, indent=0)
        f.write("\n")
    print("wrote", GOLDEN)
