"""GPU: the multilinear IPA (csrc/ipa.cpp, csrc/kernels_ipa.hip) against the Python restatement (tests/ipa_ref.py) byte for
byte, then through both verifiers; Lasso and HyperPlonk over it.

Sizes and the boundaries they sit on:
  base fold      128 threads per workgroup, 8 points behind one inversion (AX_BATCH): n = 1, 2, 63, 64, 65, 257 put a
                 partial last inversion batch, a full one, a workgroup boundary and a second workgroup under test; planted
                 lanes make an identity result share an inversion batch with ordinary ones
  round trips    num_vars 10, 13, 16 go through lh_ipa_verify, which never folds bases: an independent check of every fold
                 at sizes the Python restatement is too slow for
  Hyrax          the row combination sums 64 row slices per column: (14, 1) has 128 rows and (15, 2) 128 rows of 256 entries
                 (more rows than slices, one workgroup of columns), the byte shapes 1 to 4 rows; the commit of (14, 1) is
                 128 MSM jobs, above the 48 the batch planner takes at a time
"""
import ctypes as C
import random

import pytest

import ipa_ref as ir
from test_ipa_cpu import (ipa_check, ipa_batch_check, _queries, hyrax_check, hyrax_batch_check, HYRAX_SHAPES)
from oracle.pyref import curve
from oracle.pyref.field import R_MOD as P
from oracle.pyref.poly import evaluate
from oracle.pyref.transcript import Keccak256Transcript as OT, TranscriptError

pytestmark = pytest.mark.gpu


def _params(hl, ctx, n):
    o_pp, o_vp = ir.trim(ir.setup(1 << n), 1 << n)
    pp = hl.Ipa.trim(hl.Ipa.setup(ctx, 1 << n), 1 << n)
    return o_pp, o_vp, pp, hl.Ipa.trim(hl.Ipa.setup(None, 1 << n), 1 << n)


def _open_both(hl, ctx, n, seed, table=None):
    rng = random.Random(seed)
    o_pp, o_vp, pp, vp = _params(hl, ctx, n)
    table = [rng.randrange(P) for _ in range(1 << n)] if table is None else table
    poly = hl.MultilinearPolynomial.new(ctx, table)
    ot, t = OT(), hl.Keccak256Transcript()
    o_comm, comm = ir.commit(o_pp, table), hl.Ipa.commit(pp, poly)
    assert comm == o_comm
    if comm is not None:  # (the all-zero table commits to the identity, which no transcript carries)
        ot.write_commitment(o_comm), t.write_commitment(comm)
    point = t.squeeze_challenges(n)
    assert point == ot.squeeze_challenges(n)
    ev = evaluate(table, point)
    ot.write_field_element(ev), t.write_field_element(ev)
    o_err = g_err = None
    try:
        ir.open_(o_pp, table, point, ev, ot)
    except TranscriptError as e:
        o_err = e
    try:
        hl.Ipa.open(pp, poly, point, t)
    except hl.TranscriptError as e:
        g_err = e
    return o_vp, vp, ot.into_proof(), t.into_proof(), o_err, g_err


def test_device_generators_equal_the_host_ones(hl, ctx):
    g_dev, h_dev = hl.Ipa.setup(ctx, 1 << 10).download()
    g_host, h_host = hl.Ipa.setup(None, 1 << 10).download()
    assert g_dev == g_host and h_dev == h_host
    assert g_dev[:5] == [ir.generator_g(i) for i in range(5)] and h_dev == ir.generator_h()


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257])
def test_g1_axpy_with_planted_lanes(hl, ctx, n):
    rng = random.Random(1000 + n)
    fb = curve.FixedBase(curve.G1_GEN)
    s = rng.randrange(2, P)
    b = [fb.mul(rng.randrange(1, P)) for _ in range(n)]
    a = [fb.mul(rng.randrange(1, P)) for _ in range(n)]
    sb = [curve.mul(p, s) for p in b]
    # planted: the doubling branch, an identity result between ordinary ones, identities on either side and on both
    plant = {0: "dbl"} if n == 1 else {0: "dbl", 1: "neg"} if n == 2 else \
        {1: "dbl", 3: "neg", 4: "a0", 5: "b0", 6: "ab0", n - 1: "neg", n - 2: "dbl"}
    for j, what in plant.items():
        if what == "dbl":
            a[j] = sb[j]
        elif what == "neg":
            a[j] = curve.neg(sb[j])
        if what in ("a0", "ab0"):
            a[j] = None
        if what in ("b0", "ab0"):
            b[j], sb[j] = None, None
    want = [curve.add(x, y) for x, y in zip(a, sb)]
    assert all(want[j] is None for j, what in plant.items() if what in ("neg", "ab0"))
    assert hl.Ipa.g1_axpy(ctx, a, b, s) == want


@pytest.mark.parametrize("s", [0, 1, P - 1])
def test_g1_axpy_edge_scalars(hl, ctx, s):
    rng = random.Random(1100)
    fb = curve.FixedBase(curve.G1_GEN)
    n = 11
    a, b = [fb.mul(rng.randrange(1, P)) for _ in range(n)], [fb.mul(rng.randrange(1, P)) for _ in range(n)]
    a[2] = b[2] if s == P - 1 else curve.neg(b[2]) if s == 1 else a[2]  # an identity result where the scalar allows one
    a[3] = curve.neg(b[3]) if s == P - 1 else b[3]                      # the doubling branch at s = +-1
    want = [curve.add(x, curve.mul(y, s)) for x, y in zip(a, b)]
    assert hl.Ipa.g1_axpy(ctx, a, b, s) == want


@pytest.mark.parametrize("n", [1, 2, 3, 6, 7])
def test_ipa_open_matches_oracle(hl, ctx, n):
    o_vp, vp, o_proof, proof, o_err, g_err = _open_both(hl, ctx, n, 500 + n)
    assert o_err is None and g_err is None
    assert proof == o_proof and len(proof) == 64 + 32 + 128 * n + 32
    ipa_check(o_vp, n, proof, ir.verify, OT)
    assert ipa_check(vp, n, proof, hl.Ipa.verify, hl.Keccak256Transcript.from_proof).remaining() == 0


def test_reference_ends_upper_half_zero_and_all_zero(hl, ctx):
    """a table whose upper half is zero makes the first L the identity: the opening ends with the TranscriptError the
    reference ends with, after the same bytes"""
    n = 4
    rng = random.Random(502)
    table = [rng.randrange(P) for _ in range(1 << (n - 1))] + [0] * (1 << (n - 1))
    for tb in (table, [0] * (1 << n)):
        _, _, o_proof, proof, o_err, g_err = _open_both(hl, ctx, n, 503, table=tb)
        assert o_err is not None and g_err is not None
        assert "Invalid elliptic curve point encoding" in str(o_err) and "Invalid elliptic curve point encoding" in str(g_err)
        assert proof == o_proof


@pytest.mark.parametrize("n", [10, 13, 16])
def test_ipa_round_trip_through_the_host_verifier(hl, ctx, n):
    rng = random.Random(1200 + n)
    params = hl.Ipa.setup(ctx, 1 << n)
    pp = hl.Ipa.trim(params, 1 << n)
    table = [rng.randrange(P) for _ in range(1 << n)]
    poly = hl.MultilinearPolynomial.new(ctx, table)
    t = hl.Keccak256Transcript()
    hl.Ipa.batch_commit_and_write(pp, [poly], t)
    point = t.squeeze_challenges(n)
    ev = evaluate(table, point)
    t.write_field_element(ev)
    hl.Ipa.open(pp, poly, point, t)
    proof = t.into_proof()
    assert len(proof) == 64 + 32 + 128 * n + 32
    assert ipa_check(pp, n, proof, hl.Ipa.verify, hl.Keccak256Transcript.from_proof).remaining() == 0
    bad = bytearray(proof)
    bad[64 + 31] ^= 1  # the claimed evaluation
    with pytest.raises(hl.InvalidPcsOpen, match="Invalid multilinear IPA open"):
        ipa_check(pp, n, bytes(bad), hl.Ipa.verify, hl.Keccak256Transcript.from_proof)


@pytest.mark.parametrize("n,batch", [(2, 2), (4, 3), (6, 4)])
def test_ipa_batch_open_matches_oracle(hl, ctx, n, batch):
    rng = random.Random(600 + n)
    o_pp, o_vp, pp, vp = _params(hl, ctx, n)
    tables = [[rng.randrange(P) for _ in range(1 << n)] for _ in range(batch)]
    polys = [hl.MultilinearPolynomial.new(ctx, tb) for tb in tables]
    queries = _queries(batch, batch, rng)
    ot, t = OT(), hl.Keccak256Transcript()
    assert hl.Ipa.batch_commit_and_write(pp, polys, t) == ir.batch_commit_and_write(o_pp, tables, ot)
    points = [t.squeeze_challenges(n) for _ in range(batch)]
    assert points == [ot.squeeze_challenges(n) for _ in range(batch)]
    values = [evaluate(tables[i], points[j]) for i, j in queries]
    ot.write_field_elements(values), t.write_field_elements(values)
    ir.batch_open(o_pp, n, tables, points, [ir.Evaluation(i, j, v) for (i, j), v in zip(queries, values)], ot)
    hl.Ipa.batch_open(pp, n, polys, points, [hl.Evaluation(i, j, v) for (i, j), v in zip(queries, values)], t)
    proof = t.into_proof()
    assert proof == ot.into_proof()
    mk = lambda i, j, v: hl.Evaluation(i, j, v)
    r = ipa_batch_check(vp, n, batch, batch, queries, proof, hl.Ipa.batch_verify, hl.Keccak256Transcript.from_proof, mk)
    assert r.remaining() == 0
    ipa_batch_check(o_vp, n, batch, batch, queries, proof, ir.batch_verify, OT, ir.Evaluation)


def test_commit_against_a_prefix_and_param_errors(hl, ctx):
    n = 5
    rng = random.Random(77)
    params = hl.Ipa.setup(ctx, 1 << n)
    table = [rng.randrange(P) for _ in range(1 << (n - 2))]
    small = hl.MultilinearPolynomial.new(ctx, table)
    assert hl.Ipa.commit(hl.Ipa.trim(params, 1 << n), small) == ir.commit(ir.setup(1 << n), table)
    big = hl.MultilinearPolynomial.new(ctx, [1] * (1 << n))
    with pytest.raises(hl.InvalidPcsParam, match="Too many variates of poly to commit"):
        hl.Ipa.commit(hl.Ipa.trim(params, 1 << (n - 1)), big)
    with pytest.raises(hl.InvalidPcsParam, match="Too many variates of poly to open"):
        hl.Ipa.open(hl.Ipa.trim(params, 1 << (n - 1)), big, [1] * n, hl.Keccak256Transcript())
    host_pp = hl.Ipa.trim(hl.Ipa.setup(None, 1 << n), 1 << n)
    host_pp.ctx = ctx
    with pytest.raises(hl.ArgumentError, match="no device bases"):  # a param set up without a ctx is a verifier's
        hl.Ipa.commit(host_pp, big)


@pytest.mark.parametrize("kind,c,l,n", [("range", 2, 3, 4), ("and", 2, 4, 3), ("xor", 2, 4, 6)])
def test_lasso_over_ipa_matches_oracle(hl, ctx, kind, c, l, n):
    import array
    from oracle.pyref import lasso as o_lasso
    rng = random.Random(700 + n)
    nv = max(n, l)
    spec = o_lasso.range_table(c, l) if kind == "range" else o_lasso.bitwise_table(
        o_lasso.SUBTABLE_AND if kind == "and" else o_lasso.SUBTABLE_XOR, c, l)
    table = hl.LassoTable.range(c, l) if kind == "range" else hl.LassoTable.bitwise(
        hl.SUBTABLE_AND if kind == "and" else hl.SUBTABLE_XOR, c, l)
    dims = [[rng.randrange(1 << l) for _ in range(1 << n)] for _ in range(c)]
    o_pp, o_vp, pp, vp = _params(hl, ctx, nv)
    ot = OT()
    o_lasso.prove(o_pp, spec, dims, ot, pcs=ir)
    t = hl.Keccak256Transcript()
    hl.lasso_prove(pp, table, n, [ctx.upload(array.array("I", d).tobytes()) for d in dims], t)
    proof = t.into_proof()
    assert proof == ot.into_proof()
    o_lasso.verify(o_vp, spec, n, OT(proof), pcs=ir)
    hl.lasso_verify(vp, table, n, hl.Keccak256Transcript.from_proof(proof))
    bad = bytearray(proof)
    bad[len(bad) // 2] ^= 8
    with pytest.raises(hl.Error):
        hl.lasso_verify(vp, table, n, hl.Keccak256Transcript.from_proof(bytes(bad)))


@pytest.mark.parametrize("num_vars,with_lookup", [(3, False), (4, True), (6, True)])
def test_hyperplonk_over_ipa_matches_oracle(hl, ctx, num_vars, with_lookup):
    from halo2_lasso_amd import hyperplonk as g_hp
    from oracle.pyref import hyperplonk as o_hp
    from test_gpu_hyperplonk import _circuit
    o_info, g_info, instances, witness = _circuit(hl, num_vars, with_lookup, 900 + num_vars)
    o_pcs_pp, _, pcs_pp, pcs_vp = _params(hl, ctx, num_vars)
    o_pp = o_hp.preprocess((o_pcs_pp, o_pcs_pp), o_info, ir)
    g_pp, g_vp = g_hp.HyperPlonk.preprocess(pcs_pp, g_info, pcs_vp)
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
    params = hl.Ipa.setup(ctx, 8)
    poly = ctx.upload(b"".join(hl.fr_to_bytes(v) for v in range(8)))
    pts = ctx.alloc(64 * 4)
    out, fr3, tr = _ffi.lh_g1(), (_ffi.lh_fr * 3)(), hl.Keccak256Transcript()
    ptrs, ev = (C.c_void_p * 1)(poly.ptr), (_ffi.lh_evaluation * 1)()
    tbl = hl.LassoTable.range(2, 2).to_c()
    pts4 = (_ffi.lh_g1 * 4)()
    bad = [
        lib.lh_ipa_param_download(None, params.h, C.create_string_buffer(64 * 8), None),
        lib.lh_ipa_batch_commit(None, params.h, 8, ptrs, 1, 3, C.byref(out)),
        lib.lh_ipa_batch_commit(h, None, 8, ptrs, 1, 3, C.byref(out)),
        lib.lh_ipa_batch_commit(h, params.h, 8, None, 1, 3, C.byref(out)),
        lib.lh_ipa_batch_commit(h, params.h, 8, (C.c_void_p * 1)(None), 1, 3, C.byref(out)),
        lib.lh_ipa_batch_commit(h, params.h, 8, ptrs, 1, 3, None),
        lib.lh_ipa_open(None, params.h, 8, poly.ptr, 3, fr3, tr.p), lib.lh_ipa_open(h, None, 8, poly.ptr, 3, fr3, tr.p),
        lib.lh_ipa_open(h, params.h, 8, None, 3, fr3, tr.p), lib.lh_ipa_open(h, params.h, 8, poly.ptr, 3, None, tr.p),
        lib.lh_ipa_open(h, params.h, 8, poly.ptr, 3, fr3, None),
        lib.lh_ipa_batch_open(None, params.h, 8, 3, ptrs, 1, fr3, 1, ev, 1, tr.p),
        lib.lh_ipa_batch_open(h, None, 8, 3, ptrs, 1, fr3, 1, ev, 1, tr.p),
        lib.lh_ipa_batch_open(h, params.h, 8, 3, None, 1, fr3, 1, ev, 1, tr.p),
        lib.lh_ipa_batch_open(h, params.h, 8, 3, ptrs, 1, None, 1, ev, 1, tr.p),
        lib.lh_ipa_batch_open(h, params.h, 8, 3, ptrs, 1, fr3, 1, None, 1, tr.p),
        lib.lh_ipa_batch_open(h, params.h, 8, 3, ptrs, 1, fr3, 1, ev, 1, None),
        lib.lh_ipa_batch_open(h, params.h, 8, 3, (C.c_void_p * 1)(None), 1, fr3, 1, ev, 1, tr.p),
        lib.lh_hyrax_batch_commit(None, params.h, 8, 1, ptrs, 1, 3, pts4), lib.lh_hyrax_batch_commit(h, None, 8, 1, ptrs, 1, 3, pts4),
        lib.lh_hyrax_batch_commit(h, params.h, 8, 1, None, 1, 3, pts4),
        lib.lh_hyrax_batch_commit(h, params.h, 8, 1, (C.c_void_p * 1)(None), 1, 3, pts4),
        lib.lh_hyrax_batch_commit(h, params.h, 8, 1, ptrs, 1, 3, None),
        lib.lh_hyrax_open(None, params.h, 8, 1, poly.ptr, 3, fr3, tr.p), lib.lh_hyrax_open(h, None, 8, 1, poly.ptr, 3, fr3, tr.p),
        lib.lh_hyrax_open(h, params.h, 8, 1, None, 3, fr3, tr.p), lib.lh_hyrax_open(h, params.h, 8, 1, poly.ptr, 3, None, tr.p),
        lib.lh_hyrax_open(h, params.h, 8, 1, poly.ptr, 3, fr3, None),
        lib.lh_hyrax_batch_open(None, params.h, 8, 1, 3, ptrs, 1, fr3, 1, ev, 1, tr.p),
        lib.lh_hyrax_batch_open(h, None, 8, 1, 3, ptrs, 1, fr3, 1, ev, 1, tr.p),
        lib.lh_hyrax_batch_open(h, params.h, 8, 1, 3, None, 1, fr3, 1, ev, 1, tr.p),
        lib.lh_hyrax_batch_open(h, params.h, 8, 1, 3, (C.c_void_p * 1)(None), 1, fr3, 1, ev, 1, tr.p),
        lib.lh_hyrax_batch_open(h, params.h, 8, 1, 3, ptrs, 1, None, 1, ev, 1, tr.p),
        lib.lh_hyrax_batch_open(h, params.h, 8, 1, 3, ptrs, 1, fr3, 1, None, 1, tr.p),
        lib.lh_hyrax_batch_open(h, params.h, 8, 1, 3, ptrs, 1, fr3, 1, ev, 1, None),
        lib.lh_g1_axpy(None, pts.ptr, pts.ptr, 4, fr3, pts.ptr), lib.lh_g1_axpy(h, None, pts.ptr, 4, fr3, pts.ptr),
        lib.lh_g1_axpy(h, pts.ptr, None, 4, fr3, pts.ptr), lib.lh_g1_axpy(h, pts.ptr, pts.ptr, 4, None, pts.ptr),
        lib.lh_g1_axpy(h, pts.ptr, pts.ptr, 4, fr3, None),
        lib.lh_lasso_prove_ipa(None, params.h, 8, C.byref(tbl), 2, ptrs, tr.p),
        lib.lh_lasso_prove_ipa(h, None, 8, C.byref(tbl), 2, ptrs, tr.p),
        lib.lh_lasso_prove_ipa(h, params.h, 8, None, 2, ptrs, tr.p),
        lib.lh_lasso_prove_ipa(h, params.h, 8, C.byref(tbl), 2, None, tr.p),
        lib.lh_lasso_prove_ipa(h, params.h, 8, C.byref(tbl), 2, ptrs, None),
        lib.lh_hyperplonk_prove_ipa(None, params.h, 8, None, None, None, tr.p),
        lib.lh_hyperplonk_prove_ipa(h, None, 8, None, None, None, tr.p),
        lib.lh_hyperplonk_prove_ipa(h, params.h, 8, None, None, None, tr.p),
        lib.lh_hyperplonk_prove_phases_ipa(None, params.h, 8, None, 0, None, None, None, None, tr.p),
        lib.lh_hyperplonk_prove_phases_ipa(h, None, 8, None, 0, None, None, None, None, tr.p),
        lib.lh_hyperplonk_prove_phases_ipa(h, params.h, 8, None, 0, None, None, None, None, tr.p),
    ]
    assert bad == [_ffi.LH_ERR_ARG] * len(bad), bad
    assert lib.lh_g1_axpy(h, None, None, 0, fr3, None) == _ffi.LH_OK
    assert hl.Ipa.commit(hl.Ipa.trim(params, 8), hl.MultilinearPolynomial(ctx, poly, 3)) is not None


# ------------------------------------------------------------------ Hyrax
def _hyrax_params(hl, ctx, n, batch_size):
    o_pp, o_vp = ir.hyrax_trim(ir.hyrax_setup(1 << n, batch_size), 1 << n, batch_size)
    pp = hl.Hyrax.trim(hl.Hyrax.setup(ctx, 1 << n, batch_size), 1 << n, batch_size)
    return o_pp, o_vp, pp, hl.Hyrax.trim(hl.Hyrax.setup(None, 1 << n, batch_size), 1 << n, batch_size)


@pytest.mark.parametrize("n,batch_size", HYRAX_SHAPES)
def test_hyrax_commit_and_open_match_oracle(hl, ctx, n, batch_size):
    rng = random.Random(1300 + 10 * n + batch_size)
    o_pp, o_vp, pp, vp = _hyrax_params(hl, ctx, n, batch_size)
    table = [rng.randrange(P) for _ in range(1 << n)]
    poly = hl.MultilinearPolynomial.new(ctx, table)
    ot, t = OT(), hl.Keccak256Transcript()
    assert hl.Hyrax.commit(pp, poly) == ir.hyrax_commit(o_pp, table)
    assert hl.Hyrax.batch_commit_and_write(pp, [poly], t) == ir.hyrax_batch_commit_and_write(o_pp, [table], ot)
    point = t.squeeze_challenges(n)
    assert point == ot.squeeze_challenges(n)
    ev = evaluate(table, point)
    ot.write_field_element(ev), t.write_field_element(ev)
    ir.hyrax_open(o_pp, table, point, ev, ot)
    hl.Hyrax.open(pp, poly, point, t)
    proof = t.into_proof()
    assert proof == ot.into_proof() and len(proof) == 64 * o_pp.num_chunks + 32 + 128 * o_pp.row_num_vars + 32
    hyrax_check(o_vp, n, proof, ir.hyrax_verify, OT)
    assert hyrax_check(vp, n, proof, hl.Hyrax.verify, hl.Keccak256Transcript.from_proof).remaining() == 0


@pytest.mark.parametrize("n,batch_size", HYRAX_SHAPES)
def test_hyrax_batch_commit_and_batch_open_match_oracle(hl, ctx, n, batch_size):
    rng = random.Random(1400 + 10 * n + batch_size)
    batch = min(batch_size, 3) + 1
    o_pp, o_vp, pp, vp = _hyrax_params(hl, ctx, n, batch_size)
    tables = [[rng.randrange(P) for _ in range(1 << n)] for _ in range(batch)]
    polys = [hl.MultilinearPolynomial.new(ctx, tb) for tb in tables]
    queries = _queries(batch, 2, rng)
    ot, t = OT(), hl.Keccak256Transcript()
    assert hl.Hyrax.batch_commit_and_write(pp, polys, t) == ir.hyrax_batch_commit_and_write(o_pp, tables, ot)
    points = [t.squeeze_challenges(n) for _ in range(2)]
    assert points == [ot.squeeze_challenges(n) for _ in range(2)]
    values = [evaluate(tables[i], points[j]) for i, j in queries]
    ot.write_field_elements(values), t.write_field_elements(values)
    ir.hyrax_batch_open(o_pp, n, tables, points, [ir.Evaluation(i, j, v) for (i, j), v in zip(queries, values)], ot)
    hl.Hyrax.batch_open(pp, n, polys, points, [hl.Evaluation(i, j, v) for (i, j), v in zip(queries, values)], t)
    proof = t.into_proof()
    assert proof == ot.into_proof()
    mk = lambda i, j, v: hl.Evaluation(i, j, v)
    r = hyrax_batch_check(vp, n, batch, 2, queries, proof, hl.Hyrax.batch_verify, hl.Keccak256Transcript.from_proof, mk)
    assert r.remaining() == 0
    hyrax_batch_check(o_vp, n, batch, 2, queries, proof, ir.hyrax_batch_verify, OT, ir.Evaluation)


@pytest.mark.parametrize("n,batch_size", [(14, 1), (15, 2)])
def test_hyrax_at_size_through_the_host_verifier(hl, ctx, n, batch_size):
    rng = random.Random(1500 + n)
    pp = hl.Hyrax.trim(hl.Hyrax.setup(ctx, 1 << n, batch_size), 1 << n, batch_size)
    assert pp.num_chunks == 128
    table = [rng.randrange(P) for _ in range(1 << n)]
    poly = hl.MultilinearPolynomial.new(ctx, table)
    t = hl.Keccak256Transcript()
    comm = hl.Hyrax.batch_commit_and_write(pp, [poly], t)[0]
    for r in (0, 77, 127):  # rows against the IPA commit of the same entries
        row = hl.MultilinearPolynomial.new(ctx, table[r << pp.row_num_vars:(r + 1) << pp.row_num_vars])
        assert comm[r] == hl.Ipa.commit(hl.Ipa.trim(pp.params, 1 << pp.row_num_vars), row)
    point = t.squeeze_challenges(n)
    ev = evaluate(table, point)
    t.write_field_element(ev)
    hl.Hyrax.open(pp, poly, point, t)
    proof = t.into_proof()
    assert len(proof) == 64 * 128 + 32 + 128 * pp.row_num_vars + 32
    assert hyrax_check(pp, n, proof, hl.Hyrax.verify, hl.Keccak256Transcript.from_proof).remaining() == 0
    bad = bytearray(proof)
    bad[64 * 128 + 31] ^= 1  # the claimed evaluation
    with pytest.raises(hl.InvalidPcsOpen, match="Invalid multilinear IPA open"):
        hyrax_check(pp, n, bytes(bad), hl.Hyrax.verify, hl.Keccak256Transcript.from_proof)
