"""GPU: Gemini over univariate KZG and the batched univariate KZG opening (csrc/gemini.cpp, csrc/kernels_gemini.hip)
against the Python restatement (tests/gemini_ref.py) byte for byte, then through both verifiers.

One-variable openings and the all-zero table end in the reference with a TranscriptError - the identity commitment
cannot be written (util/transcript.rs:172-179; gemini_ref's docstring) - and must end the same way here, with the same
bytes written before it.

Thresholds of the new kernels and the sizes that sit on each side of them:
  GM_TAIL_IN = 1024   folds of a table of <= 2^10 entries run in the resident tail alone, larger ones stream first
                      (folds compared at n = 9, 10, 11, 12 against field arithmetic in Python)
  256 chunks of 64    a suffix Horner lane of <= 16384 coefficients has one chunk per scan thread, longer ones several
                      (single-point openings at 16384, 16385 and 40000 coefficients against the trapdoor form of the proof)
  1024 blocks of 256  an even/odd evaluation of <= 2^19 coefficients visits one pair per thread, longer ones several
                      (n = 19 and n = 20 against Horner in Python)
"""
import ctypes as C
import random

import pytest

import gemini_ref as gr
from test_gemini_cpu import (gemini_check, gemini_batch_check, ukzg_batch_check, UKZG_SHAPES, _queries, _tamperings)
from oracle.pyref import curve, zeromorph as o_zm
from oracle.pyref.field import R_MOD as P
from oracle.pyref.poly import evaluate
from oracle.pyref.transcript import Keccak256Transcript as OT, TranscriptError

pytestmark = pytest.mark.gpu


def _params(hl, ctx, s, size, poly_size):
    o_pp, o_vp = gr.trim(gr.setup(s, size), poly_size)
    pp = hl.Gemini.trim(hl.Gemini.setup(ctx, s, size), poly_size)
    return o_pp, o_vp, pp, hl.GeminiVerifierParam.setup(s)


def _open_both(hl, ctx, n, extra, seed, table=None):
    rng = random.Random(seed)
    s = rng.randrange(1, P)
    o_pp, o_vp, pp, vp = _params(hl, ctx, s, (1 << n) + extra, 1 << n)
    table = [rng.randrange(P) for _ in range(1 << n)] if table is None else table
    poly = hl.MultilinearPolynomial.new(ctx, table)
    ot, t = OT(), hl.Keccak256Transcript()
    o_comm = gr.batch_commit_and_write(o_pp, [table], ot)[0]
    comm = hl.Gemini.batch_commit_and_write(pp, [poly], t)[0]
    assert comm == o_comm
    point = t.squeeze_challenges(n)
    assert point == ot.squeeze_challenges(n)
    ev = evaluate(table, point)
    ot.write_field_element(ev), t.write_field_element(ev)
    o_err = g_err = None
    try:
        gr.open_(o_pp, table, point, ev, ot)
    except TranscriptError as e:
        o_err = e
    try:
        hl.Gemini.open(pp, poly, point, t)
    except hl.TranscriptError as e:
        g_err = e
    return o_vp, vp, ot.into_proof(), t.into_proof(), o_err, g_err


def test_gemini_commit_equals_zeromorph_commit(hl, ctx):
    n = 7
    rng = random.Random(1)
    s = rng.randrange(1, P)
    params = hl.Gemini.setup(ctx, s, (1 << n) + 3)
    tables = [[rng.randrange(P) for _ in range(1 << n)] for _ in range(3)]
    polys = [hl.MultilinearPolynomial.new(ctx, tb) for tb in tables]
    g = hl.Gemini.batch_commit(hl.Gemini.trim(params, 1 << n), polys)
    assert g == hl.Zeromorph.batch_commit(hl.Zeromorph.trim(params, 1 << n), polys)
    o_pp, _ = gr.trim(gr.setup(s, 1 << n), 1 << n)
    assert g == [gr.commit(o_pp, tb) for tb in tables]
    with pytest.raises(hl.InvalidPcsParam, match="Too large degree of poly to commit"):
        hl.Gemini.batch_commit(hl.Gemini.trim(params, 1 << (n - 1)), polys)
    with pytest.raises(hl.InvalidPcsParam, match="Too large degree of poly to open"):
        hl.Gemini.open(hl.Gemini.trim(params, 1 << (n - 1)), polys[0], [1] * n, hl.Keccak256Transcript())


@pytest.mark.parametrize("n,extra", [(2, 0), (3, 5), (6, 0), (7, 0), (10, 3)])
def test_gemini_open_matches_oracle(hl, ctx, n, extra):
    o_vp, vp, o_proof, proof, o_err, g_err = _open_both(hl, ctx, n, extra, 500 + n)
    assert o_err is None and g_err is None
    assert proof == o_proof and len(proof) == 64 + 32 + 96 * n + 64
    gemini_check(o_vp, n, proof, gr.verify, OT)
    t = gemini_check(vp, n, proof, hl.Gemini.verify, hl.Keccak256Transcript.from_proof)
    assert t.remaining() == 0
    for what, bad in _tamperings(proof, 64).items():
        with pytest.raises(hl.InvalidPcsOpen, match="Invalid univariate KZG open"):
            gemini_check(vp, n, bad, hl.Gemini.verify, hl.Keccak256Transcript.from_proof)


def test_gemini_open_of_one_variable_ends_as_the_reference_does(hl, ctx):
    """(n, extra) = (1, 0): fs[0] div (X^2 - beta^2) is zero, [q] is the identity, write_commitment refuses it"""
    _, _, o_proof, proof, o_err, g_err = _open_both(hl, ctx, 1, 0, 501)
    assert o_err is not None and g_err is not None
    assert "Invalid elliptic curve point encoding" in str(o_err) and "Invalid elliptic curve point encoding" in str(g_err)
    assert proof == o_proof and len(proof) == 64 + 32 + 32


def test_gemini_zero_table_and_upper_half_zero(hl, ctx):
    n = 5
    rng = random.Random(502)
    o_pp, _, pp, _ = _params(hl, ctx, rng.randrange(1, P), 1 << n, 1 << n)
    zero, point = hl.MultilinearPolynomial.new(ctx, [0] * (1 << n)), [rng.randrange(P) for _ in range(n)]
    assert hl.Gemini.commit(pp, zero) is None and gr.commit(o_pp, [0] * (1 << n)) is None  # the identity: commits without error
    ot, t = OT(), hl.Keccak256Transcript()
    with pytest.raises(TranscriptError, match="Invalid elliptic curve point encoding"):
        gr.open_(o_pp, [0] * (1 << n), point, 0, ot)
    with pytest.raises(hl.TranscriptError, match="Invalid elliptic curve point encoding"):
        hl.Gemini.open(pp, zero, point, t)  # the first fold commitment is the identity: it cannot be written, there or here
    assert t.into_proof() == ot.into_proof() == b""
    rng = random.Random(503)
    table = [rng.randrange(P) for _ in range(1 << (n - 1))] + [0] * (1 << (n - 1))
    o_vp, vp, o_proof, proof, o_err, g_err = _open_both(hl, ctx, n, 0, 504, table=table)
    assert o_err is None and g_err is None and proof == o_proof
    gemini_check(vp, n, proof, hl.Gemini.verify, hl.Keccak256Transcript.from_proof)
    gemini_check(o_vp, n, proof, gr.verify, OT)


@pytest.mark.parametrize("n,batch", [(2, 2), (4, 3), (8, 4)])
def test_gemini_batch_open_matches_oracle(hl, ctx, n, batch):
    rng = random.Random(600 + n)
    s = rng.randrange(1, P)
    o_pp, o_vp, pp, vp = _params(hl, ctx, s, 1 << n, 1 << n)
    tables = [[rng.randrange(P) for _ in range(1 << n)] for _ in range(batch)]
    polys = [hl.MultilinearPolynomial.new(ctx, tb) for tb in tables]
    queries = _queries(batch, batch, rng)
    ot, t = OT(), hl.Keccak256Transcript()
    assert hl.Gemini.batch_commit_and_write(pp, polys, t) == gr.batch_commit_and_write(o_pp, tables, ot)
    points = [t.squeeze_challenges(n) for _ in range(batch)]
    assert points == [ot.squeeze_challenges(n) for _ in range(batch)]
    values = [evaluate(tables[i], points[j]) for i, j in queries]
    ot.write_field_elements(values), t.write_field_elements(values)
    gr.batch_open(o_pp, n, tables, points, [gr.Evaluation(i, j, v) for (i, j), v in zip(queries, values)], ot)
    hl.Gemini.batch_open(pp, n, polys, points, [hl.Evaluation(i, j, v) for (i, j), v in zip(queries, values)], t)
    proof = t.into_proof()
    assert proof == ot.into_proof()
    mk = lambda i, j, v: hl.Evaluation(i, j, v)
    r = gemini_batch_check(vp, n, batch, queries, proof, hl.Gemini.batch_verify, hl.Keccak256Transcript.from_proof, mk)
    assert r.remaining() == 0
    gemini_batch_check(o_vp, n, batch, queries, proof, gr.batch_verify, OT, gr.Evaluation)
    bad = bytearray(proof)
    bad[64 * batch + 31] ^= 1
    with pytest.raises(hl.Error):
        gemini_batch_check(vp, n, batch, queries, bytes(bad), hl.Gemini.batch_verify, hl.Keccak256Transcript.from_proof, mk)


@pytest.mark.parametrize("shape", sorted(UKZG_SHAPES))
def test_ukzg_batch_open_matches_oracle(hl, ctx, shape):
    """mixed point sets, polys of different lengths, a duplicated pair, one set only (kzg.rs:301-354)"""
    lens, npts, queries = UKZG_SHAPES[shape]
    rng = random.Random(800 + len(lens))
    s = rng.randrange(1, P)
    o_pp, o_vp = gr.trim(gr.setup(s, max(lens) + 2), max(lens))
    pp = hl.UnivariateKzg.trim(hl.UnivariateKzg.setup(ctx, s, max(lens) + 2), max(lens))
    vp = hl.UnivariateKzgVerifierParam.setup(s)
    coeffs = [[rng.randrange(P) for _ in range(m)] for m in lens]
    polys = [hl.UnivariatePolynomial.from_ints(ctx, cf) for cf in coeffs]
    ot, t = OT(), hl.Keccak256Transcript()
    o_comms = [gr.ukzg_commit(o_pp, cf) for cf in coeffs]
    assert hl.UnivariateKzg.batch_commit_and_write(pp, polys, t) == o_comms
    ot.write_commitments(o_comms)
    points = t.squeeze_challenges(npts)
    assert points == ot.squeeze_challenges(npts)
    values = [gr.poly_eval(coeffs[i], points[j]) for i, j in queries]
    ot.write_field_elements(values), t.write_field_elements(values)
    gr.ukzg_batch_open(o_pp, coeffs, points, [gr.Evaluation(i, j, v) for (i, j), v in zip(queries, values)], ot)
    hl.UnivariateKzg.batch_open(pp, polys, points, [hl.Evaluation(i, j, v) for (i, j), v in zip(queries, values)], t)
    proof = t.into_proof()
    assert proof == ot.into_proof()
    mk = lambda i, j, v: hl.Evaluation(i, j, v)
    r = ukzg_batch_check(vp, len(lens), npts, queries, proof, hl.UnivariateKzg.batch_verify,
                         hl.Keccak256Transcript.from_proof, mk)
    assert r.remaining() == 0
    ukzg_batch_check(o_vp, len(lens), npts, queries, proof, gr.ukzg_batch_verify, OT, gr.Evaluation)
    for what, bad in _tamperings(proof, 64 * len(lens)).items():
        with pytest.raises(hl.InvalidPcsOpen, match="Invalid univariate KZG open"):
            ukzg_batch_check(vp, len(lens), npts, queries, bad, hl.UnivariateKzg.batch_verify,
                             hl.Keccak256Transcript.from_proof, mk)
    with pytest.raises(hl.InvalidPcsParam, match="Too large degree of poly to open"):
        hl.UnivariateKzg.batch_open(hl.UnivariateKzg.trim(pp.params, max(lens) - 1), polys, points,
                                    [hl.Evaluation(i, j, v) for (i, j), v in zip(queries, values)], hl.Keccak256Transcript())


@pytest.mark.parametrize("n", [2, 9, 10, 11, 12])
def test_gemini_folds_on_both_sides_of_the_resident_tail(hl, ctx, n):
    rng = random.Random(900 + n)
    table = [rng.randrange(P) for _ in range(1 << n)]
    point = [rng.randrange(P) for _ in range(n)]
    got = hl.Gemini.folds(ctx, hl.MultilinearPolynomial.new(ctx, table), point)
    assert got == gr.gemini_folds(table, point)[1:]


@pytest.mark.parametrize("length", [1, 2, 63, 64, 65, 16384, 16385, 40000])
def test_ukzg_open_on_both_sides_of_the_chunked_scan(hl, ctx, length):
    """the proof of a single-point opening is ((f(s) - f(x)) / (s - x)) G: field arithmetic and one fixed-base
    multiplication say what the device's division and MSM must give"""
    rng = random.Random(1000 + length)
    s = rng.randrange(1, P)
    pp = hl.UnivariateKzg.trim(hl.UnivariateKzg.setup(ctx, s, length), length)
    coeffs = [rng.randrange(P) for _ in range(length)]
    poly = hl.UnivariatePolynomial.from_ints(ctx, coeffs)
    t = hl.Keccak256Transcript()
    comm = hl.UnivariateKzg.batch_commit_and_write(pp, [poly], t)[0]
    fb = curve.FixedBase(curve.G1_GEN)
    f_s = gr.poly_eval(coeffs, s)
    assert comm == fb.mul(f_s)
    x = t.squeeze_challenge()
    f_x = gr.poly_eval(coeffs, x)
    t.write_field_element(f_x)
    if length == 1:  # the quotient is zero: the identity cannot be written (as in the reference)
        with pytest.raises(hl.TranscriptError):
            hl.UnivariateKzg.open(pp, poly, x, t)
        return
    hl.UnivariateKzg.open(pp, poly, x, t)
    proof = t.into_proof()
    want = fb.mul((f_s - f_x) * pow(s - x, P - 2, P) % P)
    assert proof[-64:] == want[0].to_bytes(32, "big") + want[1].to_bytes(32, "big")
    r = hl.Keccak256Transcript.from_proof(proof)
    hl.UnivariateKzg.verify(hl.UnivariateKzgVerifierParam.setup(s), r.read_commitment(), r.squeeze_challenge(),
                            r.read_field_element(), r)


def _large_open(hl, ctx, n, seed):
    rng = random.Random(seed)
    s = rng.randrange(1, P)
    pp = hl.Gemini.trim(hl.Gemini.setup(ctx, s, 1 << n), 1 << n)
    table = [rng.randrange(P) for _ in range(1 << n)]
    poly = hl.MultilinearPolynomial.new(ctx, table)
    t = hl.Keccak256Transcript()
    hl.Gemini.batch_commit_and_write(pp, [poly], t)
    point = t.squeeze_challenges(n)
    ev = evaluate(table, point)
    t.write_field_element(ev)
    hl.Gemini.open(pp, poly, point, t)
    return s, pp, table, poly, point, t.into_proof()


@pytest.mark.parametrize("n", [19, 20])
def test_gemini_large_open(hl, ctx, n):
    """(a few seconds each on an MI355X, most of it Python: not marked heavy)  Past what the restatement's MSMs finish in: the library's verifier accepts the opening (two pairings that fix [q]
    and pi), the fold commitments are Zeromorph's commitments of the downloaded folds, the written evaluations are
    Horner's in Python"""
    s, pp, table, poly, point, proof = _large_open(hl, ctx, n, 1100 + n)
    assert len(proof) == 64 + 32 + 96 * n + 64
    r = gemini_check(hl.GeminiVerifierParam.setup(s), n, proof, hl.Gemini.verify, hl.Keccak256Transcript.from_proof)
    assert r.remaining() == 0
    folds = hl.Gemini.folds(ctx, poly, point)
    assert folds[0][:64] == gr.gemini_folds(table[:128], point[:1] + [0])[1]
    zpp = hl.Zeromorph.trim(pp.params, 1 << n)
    want = [hl.Zeromorph.commit(zpp, hl.MultilinearPolynomial.new(ctx, f)) for f in folds]
    rd = hl.Keccak256Transcript.from_proof(proof)
    rd.read_commitments(1), rd.squeeze_challenges(n), rd.read_field_element()
    assert rd.read_commitments(n - 1) == want
    beta = rd.squeeze_challenge()
    evs = rd.read_field_elements(n)
    assert evs[0] == gr.poly_eval(table, (-beta) % P)
    sq = gr._squares(beta, n)
    for i in (1, 2, n - 1):
        assert evs[i] == gr.poly_eval(folds[i - 1], (-sq[i]) % P)
    for what, bad in _tamperings(proof, 64).items():
        with pytest.raises(hl.InvalidPcsOpen, match="Invalid univariate KZG open"):
            gemini_check(hl.GeminiVerifierParam.setup(s), n, bad, hl.Gemini.verify, hl.Keccak256Transcript.from_proof)


@pytest.mark.parametrize("kind,c,l,n", [("range", 2, 3, 4), ("and", 2, 4, 3), ("xor", 2, 4, 6)])
def test_lasso_over_gemini_matches_oracle(hl, ctx, kind, c, l, n):
    """the geometries of test_lasso_over_zeromorph_matches_oracle with the other PCS"""
    import array
    from oracle.pyref import lasso as o_lasso
    rng = random.Random(700 + n)
    s = rng.randrange(1, P)
    nv = max(n, l)
    spec = o_lasso.range_table(c, l) if kind == "range" else o_lasso.bitwise_table(
        o_lasso.SUBTABLE_AND if kind == "and" else o_lasso.SUBTABLE_XOR, c, l)
    table = hl.LassoTable.range(c, l) if kind == "range" else hl.LassoTable.bitwise(
        hl.SUBTABLE_AND if kind == "and" else hl.SUBTABLE_XOR, c, l)
    dims = [[rng.randrange(1 << l) for _ in range(1 << n)] for _ in range(c)]
    o_pp, o_vp, pp, vp = _params(hl, ctx, s, 1 << nv, 1 << nv)
    ot = OT()
    o_lasso.prove(o_pp, spec, dims, ot, pcs=gr)
    t = hl.Keccak256Transcript()
    hl.lasso_prove(pp, table, n, [ctx.upload(array.array("I", d).tobytes()) for d in dims], t)
    proof = t.into_proof()
    assert proof == ot.into_proof()
    o_lasso.verify(o_vp, spec, n, OT(proof), pcs=gr)
    hl.lasso_verify(vp, table, n, hl.Keccak256Transcript.from_proof(proof))
    bad = bytearray(proof)
    bad[len(bad) // 2] ^= 8
    with pytest.raises(hl.Error):
        hl.lasso_verify(vp, table, n, hl.Keccak256Transcript.from_proof(bytes(bad)))


@pytest.mark.parametrize("num_vars,with_lookup", [(3, False), (4, True), (6, True)])
def test_hyperplonk_over_gemini_matches_oracle(hl, ctx, num_vars, with_lookup):
    """HyperPlonk<Gemini<UnivariateKzg<Bn256>>> (backend/hyperplonk.rs:425) at the sizes test_gpu_hyperplonk.py uses for
    Zeromorph, on vanilla_plonk and vanilla_plonk_with_lookup"""
    from halo2_lasso_amd import hyperplonk as g_hp
    from oracle.pyref import hyperplonk as o_hp
    from test_gpu_hyperplonk import _circuit
    rng = random.Random(300 + num_vars)
    s = rng.randrange(1, P)
    o_info, g_info, instances, witness = _circuit(hl, num_vars, with_lookup, 900 + num_vars)
    o_pp = o_hp.preprocess(gr.trim(gr.setup(s, 1 << num_vars), 1 << num_vars), o_info, gr)
    pcs_pp = hl.Gemini.trim(hl.Gemini.setup(ctx, s, 1 << num_vars), 1 << num_vars)
    g_pp, g_vp = g_hp.HyperPlonk.preprocess(pcs_pp, g_info, hl.GeminiVerifierParam.setup(s))
    assert g_pp.preprocess_comms == o_pp.preprocess_comms and g_pp.permutation_comms == o_pp.permutation_comms
    ot = OT()
    o_hp.prove(o_pp, instances, lambda rnd, ch: witness, ot)
    t = hl.Keccak256Transcript()
    g_hp.HyperPlonk.prove(g_pp, instances, [hl.MultilinearPolynomial.new(ctx, w) for w in witness], t)
    proof = t.into_proof()
    assert proof == ot.into_proof()
    o_hp.verify(o_pp, instances, OT(proof))
    r = hl.Keccak256Transcript.from_proof(proof)
    g_hp.HyperPlonk.verify(g_vp, instances, r)
    assert r.remaining() == 0
    bad = bytearray(proof)
    bad[len(bad) // 2] ^= 2
    with pytest.raises(hl.Error):
        g_hp.HyperPlonk.verify(g_vp, instances, hl.Keccak256Transcript.from_proof(bytes(bad)))


def test_null_arguments_of_the_prover_entry_points(hl, ctx):
    """NULL is LH_ERR_ARG at every new entry point that takes a ctx (capi.cpp NEED / NEED_N), and the ctx still works"""
    from halo2_lasso_amd import _ffi
    lib, h = ctx.lib, ctx.h
    params = hl.Gemini.setup(ctx, 7, 8)
    poly = ctx.upload(b"".join(hl.fr_to_bytes(v) for v in range(8)))
    out, fr3, tr = _ffi.lh_g1(), (_ffi.lh_fr * 3)(), hl.Keccak256Transcript()
    ptrs, lens, ev = (C.c_void_p * 1)(poly.ptr), (C.c_size_t * 1)(8), (_ffi.lh_evaluation * 1)()
    tbl = hl.LassoTable.range(2, 2).to_c()
    bad = [
        lib.lh_ukzg_batch_commit(None, params.h, 8, ptrs, lens, 1, C.byref(out)),
        lib.lh_ukzg_batch_commit(h, None, 8, ptrs, lens, 1, C.byref(out)),
        lib.lh_ukzg_batch_commit(h, params.h, 8, None, lens, 1, C.byref(out)),
        lib.lh_ukzg_batch_commit(h, params.h, 8, ptrs, None, 1, C.byref(out)),
        lib.lh_ukzg_batch_commit(h, params.h, 8, ptrs, lens, 1, None),
        lib.lh_ukzg_batch_commit(h, params.h, 8, (C.c_void_p * 1)(None), lens, 1, C.byref(out)),
        lib.lh_ukzg_open(None, params.h, 8, poly.ptr, 8, fr3, tr.p), lib.lh_ukzg_open(h, None, 8, poly.ptr, 8, fr3, tr.p),
        lib.lh_ukzg_open(h, params.h, 8, None, 8, fr3, tr.p), lib.lh_ukzg_open(h, params.h, 8, poly.ptr, 8, None, tr.p),
        lib.lh_ukzg_open(h, params.h, 8, poly.ptr, 8, fr3, None),
        lib.lh_ukzg_batch_open(None, params.h, 8, ptrs, lens, 1, fr3, 1, ev, 1, tr.p),
        lib.lh_ukzg_batch_open(h, None, 8, ptrs, lens, 1, fr3, 1, ev, 1, tr.p),
        lib.lh_ukzg_batch_open(h, params.h, 8, None, lens, 1, fr3, 1, ev, 1, tr.p),
        lib.lh_ukzg_batch_open(h, params.h, 8, ptrs, None, 1, fr3, 1, ev, 1, tr.p),
        lib.lh_ukzg_batch_open(h, params.h, 8, ptrs, lens, 1, None, 1, ev, 1, tr.p),
        lib.lh_ukzg_batch_open(h, params.h, 8, ptrs, lens, 1, fr3, 1, None, 1, tr.p),
        lib.lh_ukzg_batch_open(h, params.h, 8, ptrs, lens, 1, fr3, 1, ev, 1, None),
        lib.lh_gemini_batch_commit(None, params.h, 8, ptrs, 1, 3, C.byref(out)),
        lib.lh_gemini_batch_commit(h, None, 8, ptrs, 1, 3, C.byref(out)),
        lib.lh_gemini_batch_commit(h, params.h, 8, None, 1, 3, C.byref(out)),
        lib.lh_gemini_batch_commit(h, params.h, 8, (C.c_void_p * 1)(None), 1, 3, C.byref(out)),
        lib.lh_gemini_batch_commit(h, params.h, 8, ptrs, 1, 3, None),
        lib.lh_gemini_open(None, params.h, 8, poly.ptr, 3, fr3, tr.p), lib.lh_gemini_open(h, None, 8, poly.ptr, 3, fr3, tr.p),
        lib.lh_gemini_open(h, params.h, 8, None, 3, fr3, tr.p), lib.lh_gemini_open(h, params.h, 8, poly.ptr, 3, None, tr.p),
        lib.lh_gemini_open(h, params.h, 8, poly.ptr, 3, fr3, None),
        lib.lh_gemini_batch_open(None, params.h, 8, 3, ptrs, 1, fr3, 1, ev, 1, tr.p),
        lib.lh_gemini_batch_open(h, None, 8, 3, ptrs, 1, fr3, 1, ev, 1, tr.p),
        lib.lh_gemini_batch_open(h, params.h, 8, 3, None, 1, fr3, 1, ev, 1, tr.p),
        lib.lh_gemini_batch_open(h, params.h, 8, 3, ptrs, 1, None, 1, ev, 1, tr.p),
        lib.lh_gemini_batch_open(h, params.h, 8, 3, ptrs, 1, fr3, 1, None, 1, tr.p),
        lib.lh_gemini_batch_open(h, params.h, 8, 3, ptrs, 1, fr3, 1, ev, 1, None),
        lib.lh_gemini_folds(None, poly.ptr, 3, fr3, poly.ptr), lib.lh_gemini_folds(h, None, 3, fr3, poly.ptr),
        lib.lh_gemini_folds(h, poly.ptr, 3, None, poly.ptr), lib.lh_gemini_folds(h, poly.ptr, 3, fr3, None),
        lib.lh_lasso_prove_gemini(None, params.h, 8, C.byref(tbl), 2, ptrs, tr.p),
        lib.lh_lasso_prove_gemini(h, None, 8, C.byref(tbl), 2, ptrs, tr.p),
        lib.lh_lasso_prove_gemini(h, params.h, 8, None, 2, ptrs, tr.p),
        lib.lh_lasso_prove_gemini(h, params.h, 8, C.byref(tbl), 2, None, tr.p),
        lib.lh_lasso_prove_gemini(h, params.h, 8, C.byref(tbl), 2, ptrs, None),
        lib.lh_hyperplonk_prove_gemini(None, params.h, 8, None, None, None, tr.p),
        lib.lh_hyperplonk_prove_gemini(h, None, 8, None, None, None, tr.p),
        lib.lh_hyperplonk_prove_gemini(h, params.h, 8, None, None, None, tr.p),
        lib.lh_hyperplonk_prove_phases_gemini(None, params.h, 8, None, 0, None, None, None, None, tr.p),
        lib.lh_hyperplonk_prove_phases_gemini(h, None, 8, None, 0, None, None, None, None, tr.p),
        lib.lh_hyperplonk_prove_phases_gemini(h, params.h, 8, None, 0, None, None, None, None, tr.p),
    ]
    assert bad == [_ffi.LH_ERR_ARG] * len(bad), bad
    assert lib.lh_ukzg_batch_commit(h, params.h, 8, None, None, 0, None) == _ffi.LH_OK
    assert hl.Gemini.commit(hl.Gemini.trim(params, 8), hl.MultilinearPolynomial(ctx, poly, 3)) is not None
