"""CPU: the multilinear IPA - the Python restatement (tests/ipa_ref.py) on itself, the generator specification, and the
library's host side (host setup, lh_ipa_verify / lh_ipa_batch_verify; no GPU) on the restatement's proofs.

The shapes follow pcs/multilinear.rs run_commit_open_verify / run_batch_commit_open_verify.  A proof of one opening is
  commitment (64) | evaluation (32) | num_vars x (L (64), R (64)) | last coefficient (32).

tests/golden/ipa_generators.json was written once by `python tests/test_ipa_cpu.py` (the __main__ block below).
"""
import ctypes as C
import json
import os
import random

import pytest

if __name__ == "__main__":  # (under pytest tests/conftest.py has done this)
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ipa_ref as ir
from oracle.pyref import curve
from oracle.pyref.field import R_MOD as P, Q_MOD
from oracle.pyref.poly import evaluate
from oracle.pyref.transcript import Keccak256Transcript as OT

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ipa_generators.json")


# ------------------------------------------------------------------ proofs by the restatement
def ipa_proof(n, seed, table=None):
    rng = random.Random(seed)
    pp, vp = ir.trim(ir.setup(1 << n), 1 << n)
    table = [rng.randrange(P) for _ in range(1 << n)] if table is None else table
    t = OT()
    comm = ir.batch_commit_and_write(pp, [table], t)[0]
    point = t.squeeze_challenges(n)
    ev = evaluate(table, point)
    t.write_field_element(ev)
    ir.open_(pp, table, point, ev, t)
    return dict(n=n, table=table, comm=comm, point=point, eval=ev, proof=t.into_proof()), vp


def ipa_check(vp, n, proof, verify, from_proof):
    t = from_proof(proof)
    comm = t.read_commitments(1)[0]
    point = t.squeeze_challenges(n)
    ev = t.read_field_element()
    verify(vp, comm, point, ev, t)
    return t


def _queries(num_polys, num_points, rng):
    """every point on poly 0 (a poly opened at several points), every poly on point 0, then random pairs; unique, in order"""
    qs = [(0, j) for j in range(num_points)] + [(i, 0) for i in range(1, num_polys)]
    qs += [(rng.randrange(num_polys), rng.randrange(num_points)) for _ in range(num_polys)]
    return list(dict.fromkeys(qs))


def ipa_batch_proof(n, num_polys, num_points, seed):
    rng = random.Random(seed)
    pp, vp = ir.trim(ir.setup(1 << n), 1 << n)
    polys = [[rng.randrange(P) for _ in range(1 << n)] for _ in range(num_polys)]
    queries = _queries(num_polys, num_points, rng)
    t = OT()
    ir.batch_commit_and_write(pp, polys, t)
    points = [t.squeeze_challenges(n) for _ in range(num_points)]
    evals = [ir.Evaluation(i, j, evaluate(polys[i], points[j])) for i, j in queries]
    t.write_field_elements([e.value for e in evals])
    ir.batch_open(pp, n, polys, points, evals, t)
    return dict(n=n, polys=polys, queries=queries, proof=t.into_proof()), vp


def ipa_batch_check(vp, n, num_polys, num_points, queries, proof, batch_verify, from_proof, mk_eval):
    t = from_proof(proof)
    comms = t.read_commitments(num_polys)
    points = [t.squeeze_challenges(n) for _ in range(num_points)]
    values = t.read_field_elements(len(queries))
    batch_verify(vp, n, comms, points, [mk_eval(i, j, v) for (i, j), v in zip(queries, values)], t)
    return t


def _negate_point(proof, off):
    """the point at `off` replaced by its negative (y -> q - y: still on the curve, so it is read and reaches the check)"""
    bad = bytearray(proof)
    bad[off + 32:off + 64] = (Q_MOD - int.from_bytes(proof[off + 32:off + 64], "big")).to_bytes(32, "big")
    return bytes(bad)


def tamperings(proof, n):
    """every written item changed in turn: each L, each R, the last coefficient, the evaluation, the commitment"""
    out = {}
    for i in range(n):
        out["L%d" % i] = _negate_point(proof, 96 + 128 * i)
        out["R%d" % i] = _negate_point(proof, 96 + 128 * i + 64)
    last = bytearray(proof)
    last[-1] ^= 1
    out["last coefficient"] = bytes(last)
    ev = bytearray(proof)
    ev[64 + 31] ^= 1
    out["evaluation"] = bytes(ev)
    comm = bytearray(proof)
    comm[0:64] = (1).to_bytes(32, "big") + (2).to_bytes(32, "big")
    out["commitment"] = bytes(comm)
    return out


BATCH_SHAPES = [(2, 2, 2), (3, 3, 2), (4, 4, 3)]  # (num_vars, polys, points)


# ------------------------------------------------------------------ the generator specification
def test_generators_are_on_the_curve_distinct_and_even():
    pp = ir.setup(64)
    pts = list(pp.g) + [pp.h]
    assert all(p is not None and curve.is_on_curve(p) and 0 <= p[0] < Q_MOD and 0 < p[1] < Q_MOD for p in pts)
    assert all(p[1] % 2 == 0 for p in pts)
    assert len(set(pts)) == len(pts)


def test_generators_match_the_pinned_fixture():
    with open(GOLDEN) as f:
        gold = json.load(f)
    assert gold["domain"] == ir.DOMAIN.decode()
    assert [[hex(c) for c in ir.generator_g(i)] for i in range(5)] == gold["g"]
    assert [hex(c) for c in ir.generator_h()] == gold["h"]


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6])
def test_library_host_setup_equals_the_specification(hl, n):
    g, h = hl.Ipa.setup(None, 1 << n).download()
    want = ir.setup(1 << n)
    assert g == want.g and h == want.h


def test_setup_and_trim_arguments(hl):
    from halo2_lasso_amd import _ffi
    lib, out = _ffi.load(), C.c_void_p()
    assert lib.lh_ipa_setup(None, 1, C.byref(out)) == _ffi.LH_ERR_ARG  # num_vars = 0: h_coeffs asserts (ipa.rs:320)
    assert lib.lh_ipa_setup(None, 6, C.byref(out)) == _ffi.LH_ERR_ARG  # not a power of two (ipa.rs:99)
    params = hl.Ipa.setup(None, 8)
    assert params.size == 8 and hl.Ipa.trim(params, 4).poly_size == 4
    with pytest.raises(hl.InvalidPcsParam, match="Too many variates to trim"):
        hl.Ipa.trim(params, 16)
    with pytest.raises(ir.PcsError, match="Too many variates to trim"):
        ir.trim(ir.setup(8), 16)
    # the library checks the trim size itself too
    t = hl.Keccak256Transcript.from_proof(b"\x00" * 64)
    assert lib.lh_ipa_verify(params.h, 16, _ffi.lh_g1(), (_ffi.lh_fr * 4)(), 4, _ffi.lh_fr(), t.p) == _ffi.LH_ERR_INVALID_PCS_PARAM
    assert lib.lh_ipa_verify(params.h, 8, _ffi.lh_g1(), (_ffi.lh_fr * 4)(), 2, _ffi.lh_fr(), t.p) == _ffi.LH_ERR_ARG


# ------------------------------------------------------------------ open / verify
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6])
def test_ipa_prove_verify_by_both_verifiers(hl, n):
    d, o_vp = ipa_proof(n, 100 + n)
    assert len(d["proof"]) == 64 + 32 + 128 * n + 32
    t = ipa_check(o_vp, n, d["proof"], ir.verify, OT)
    assert t.pos == len(d["proof"])
    vp = hl.Ipa.trim(hl.Ipa.setup(None, 1 << n), 1 << n)
    r = ipa_check(vp, n, d["proof"], hl.Ipa.verify, hl.Keccak256Transcript.from_proof)
    assert r.remaining() == 0


@pytest.mark.parametrize("n", [1, 3, 5])
def test_every_tampered_item_is_rejected_by_both_verifiers(hl, n):
    d, o_vp = ipa_proof(n, 200 + n)
    vp = hl.Ipa.trim(hl.Ipa.setup(None, 1 << n), 1 << n)
    for what, bad in tamperings(d["proof"], n).items():
        with pytest.raises(ir.PcsError, match="Invalid multilinear IPA open"):
            ipa_check(o_vp, n, bad, ir.verify, OT)
        with pytest.raises(hl.InvalidPcsOpen, match="Invalid multilinear IPA open"):
            ipa_check(vp, n, bad, hl.Ipa.verify, hl.Keccak256Transcript.from_proof)


def test_verify_with_a_param_trimmed_from_a_larger_one(hl):
    d, _ = ipa_proof(3, 303)
    vp = hl.Ipa.trim(hl.Ipa.setup(None, 32), 8)
    assert ipa_check(vp, 3, d["proof"], hl.Ipa.verify, hl.Keccak256Transcript.from_proof).remaining() == 0


@pytest.mark.parametrize("n,num_polys,num_points", BATCH_SHAPES)
def test_ipa_batch_verify(hl, n, num_polys, num_points):
    d, o_vp = ipa_batch_proof(n, num_polys, num_points, 400 + n)
    assert any(sum(1 for i, _ in d["queries"] if i == k) >= 2 for k in range(num_polys))  # a poly opened at two points
    ipa_batch_check(o_vp, n, num_polys, num_points, d["queries"], d["proof"], ir.batch_verify, OT, ir.Evaluation)
    vp = hl.Ipa.trim(hl.Ipa.setup(None, 1 << n), 1 << n)
    mk = lambda i, j, v: hl.Evaluation(i, j, v)
    r = ipa_batch_check(vp, n, num_polys, num_points, d["queries"], d["proof"], hl.Ipa.batch_verify,
                        hl.Keccak256Transcript.from_proof, mk)
    assert r.remaining() == 0
    bad = bytearray(d["proof"])
    bad[64 * num_polys + 31] ^= 1  # the first evaluation
    with pytest.raises(hl.Error):
        ipa_batch_check(vp, n, num_polys, num_points, d["queries"], bytes(bad), hl.Ipa.batch_verify,
                        hl.Keccak256Transcript.from_proof, mk)
    with pytest.raises(Exception):
        ipa_batch_check(o_vp, n, num_polys, num_points, d["queries"], bytes(bad), ir.batch_verify, OT, ir.Evaluation)


def test_null_arguments_of_the_host_entry_points(hl):
    from halo2_lasso_amd import _ffi
    lib = _ffi.load()
    params = hl.Ipa.setup(None, 4)
    g1, fr2, fr, ev = _ffi.lh_g1(), (_ffi.lh_fr * 2)(), _ffi.lh_fr(), (_ffi.lh_evaluation * 1)()
    t = hl.Keccak256Transcript.from_proof(b"")
    tbl = hl.LassoTable.range(2, 2).to_c()
    bad = [
        lib.lh_ipa_setup(None, 4, None),
        lib.lh_ipa_param_download(None, None, None, C.byref(g1)),
        lib.lh_ipa_verify(None, 4, C.byref(g1), fr2, 2, C.byref(fr), t.p),
        lib.lh_ipa_verify(params.h, 4, None, fr2, 2, C.byref(fr), t.p),
        lib.lh_ipa_verify(params.h, 4, C.byref(g1), None, 2, C.byref(fr), t.p),
        lib.lh_ipa_verify(params.h, 4, C.byref(g1), fr2, 2, None, t.p),
        lib.lh_ipa_verify(params.h, 4, C.byref(g1), fr2, 2, C.byref(fr), None),
        lib.lh_ipa_batch_verify(None, 4, 2, C.byref(g1), 1, fr2, 1, ev, 1, t.p),
        lib.lh_ipa_batch_verify(params.h, 4, 2, None, 1, fr2, 1, ev, 1, t.p),
        lib.lh_ipa_batch_verify(params.h, 4, 2, C.byref(g1), 1, None, 1, ev, 1, t.p),
        lib.lh_ipa_batch_verify(params.h, 4, 2, C.byref(g1), 1, fr2, 1, None, 1, t.p),
        lib.lh_ipa_batch_verify(params.h, 4, 2, C.byref(g1), 1, fr2, 1, ev, 1, None),
        lib.lh_lasso_verify_ipa(None, 4, C.byref(tbl), 2, t.p),
        lib.lh_lasso_verify_ipa(params.h, 4, None, 2, t.p),
        lib.lh_lasso_verify_ipa(params.h, 4, C.byref(tbl), 2, None),
        lib.lh_hyperplonk_verify_ipa(None, 4, None, None, t.p),
        lib.lh_hyperplonk_verify_ipa(params.h, 4, None, None, t.p),
        lib.lh_hyperplonk_verify_phases_ipa(None, 4, None, 0, None, None, None, t.p),
        lib.lh_hyperplonk_verify_phases_ipa(params.h, 4, None, 0, None, None, None, t.p),
    ]
    assert bad == [_ffi.LH_ERR_ARG] * len(bad), bad
    assert lib.lh_ipa_param_size(None) == 0
    lib.lh_ipa_param_free(None, None)


# ------------------------------------------------------------------ Hyrax
# odd and even batch_num_vars, several rows; (2, 4) leaves the poly as a single row (hi is empty; hyrax.rs:240-244,299-301)
HYRAX_SHAPES = [(2, 1), (3, 1), (4, 3), (5, 1), (6, 4), (2, 4)]


def hyrax_proof(n, batch_size, seed):
    rng = random.Random(seed)
    pp, vp = ir.hyrax_trim(ir.hyrax_setup(1 << n, batch_size), 1 << n, batch_size)
    table = [rng.randrange(P) for _ in range(1 << n)]
    t = OT()
    comm = ir.hyrax_batch_commit_and_write(pp, [table], t)[0]
    point = t.squeeze_challenges(n)
    ev = evaluate(table, point)
    t.write_field_element(ev)
    ir.hyrax_open(pp, table, point, ev, t)
    return dict(n=n, table=table, comm=comm, point=point, eval=ev, proof=t.into_proof()), vp


def hyrax_check(vp, n, proof, verify, from_proof):
    t = from_proof(proof)
    comm = t.read_commitments(vp.num_chunks)
    point = t.squeeze_challenges(n)
    ev = t.read_field_element()
    verify(vp, comm, point, ev, t)
    return t


def hyrax_batch_proof(n, batch_size, num_polys, num_points, seed):
    rng = random.Random(seed)
    pp, vp = ir.hyrax_trim(ir.hyrax_setup(1 << n, batch_size), 1 << n, batch_size)
    polys = [[rng.randrange(P) for _ in range(1 << n)] for _ in range(num_polys)]
    queries = _queries(num_polys, num_points, rng)
    t = OT()
    ir.hyrax_batch_commit_and_write(pp, polys, t)
    points = [t.squeeze_challenges(n) for _ in range(num_points)]
    evals = [ir.Evaluation(i, j, evaluate(polys[i], points[j])) for i, j in queries]
    t.write_field_elements([e.value for e in evals])
    ir.hyrax_batch_open(pp, n, polys, points, evals, t)
    return dict(n=n, polys=polys, queries=queries, proof=t.into_proof()), vp


def hyrax_batch_check(vp, n, num_polys, num_points, queries, proof, batch_verify, from_proof, mk_eval):
    t = from_proof(proof)
    comms = [t.read_commitments(vp.num_chunks) for _ in range(num_polys)]
    points = [t.squeeze_challenges(n) for _ in range(num_points)]
    values = t.read_field_elements(len(queries))
    batch_verify(vp, n, comms, points, [mk_eval(i, j, v) for (i, j), v in zip(queries, values)], t)
    return t


def hyrax_tamperings(proof, chunks, rounds):
    """every written item changed in turn: each row commitment, the evaluation, each L, each R, the last coefficient"""
    out = {}
    for k in range(chunks):
        out["row commitment %d" % k] = _negate_point(proof, 64 * k)
    ev = bytearray(proof)
    ev[64 * chunks + 31] ^= 1
    out["evaluation"] = bytes(ev)
    base = 64 * chunks + 32
    for i in range(rounds):
        out["L%d" % i] = _negate_point(proof, base + 128 * i)
        out["R%d" % i] = _negate_point(proof, base + 128 * i + 64)
    last = bytearray(proof)
    last[-1] ^= 1
    out["last coefficient"] = bytes(last)
    return out


def _hyrax_lib_vp(hl, n, batch_size):
    return hl.Hyrax.trim(hl.Hyrax.setup(None, 1 << n, batch_size), 1 << n, batch_size)


@pytest.mark.parametrize("n,batch_size", HYRAX_SHAPES)
def test_hyrax_prove_verify_and_tampering_by_both_verifiers(hl, n, batch_size):
    d, o_vp = hyrax_proof(n, batch_size, 500 + 10 * n + batch_size)
    chunks, rounds = o_vp.num_chunks, o_vp.row_num_vars
    assert (chunks == 1) == (n == 2 and batch_size == 4)
    assert len(d["proof"]) == 64 * chunks + 32 + 128 * rounds + 32
    assert hyrax_check(o_vp, n, d["proof"], ir.hyrax_verify, OT).pos == len(d["proof"])
    vp = _hyrax_lib_vp(hl, n, batch_size)
    assert (vp.num_chunks, vp.row_num_vars) == (chunks, rounds)
    assert hyrax_check(vp, n, d["proof"], hl.Hyrax.verify, hl.Keccak256Transcript.from_proof).remaining() == 0
    for what, bad in hyrax_tamperings(d["proof"], chunks, rounds).items():
        with pytest.raises(ir.PcsError, match="Invalid multilinear IPA open"):
            hyrax_check(o_vp, n, bad, ir.hyrax_verify, OT)
        with pytest.raises(hl.InvalidPcsOpen, match="Invalid multilinear IPA open"):
            hyrax_check(vp, n, bad, hl.Hyrax.verify, hl.Keccak256Transcript.from_proof)


@pytest.mark.parametrize("n,batch_size,num_polys,num_points", [(2, 1, 2, 2), (3, 1, 3, 2), (4, 3, 3, 3), (5, 1, 2, 2),
                                                               (6, 4, 4, 3), (2, 4, 4, 2)])
def test_hyrax_batch_verify(hl, n, batch_size, num_polys, num_points):
    d, o_vp = hyrax_batch_proof(n, batch_size, num_polys, num_points, 600 + 10 * n + batch_size)
    assert any(sum(1 for i, _ in d["queries"] if i == k) >= 2 for k in range(num_polys))  # a poly opened at two points
    hyrax_batch_check(o_vp, n, num_polys, num_points, d["queries"], d["proof"], ir.hyrax_batch_verify, OT, ir.Evaluation)
    vp = _hyrax_lib_vp(hl, n, batch_size)
    mk = lambda i, j, v: hl.Evaluation(i, j, v)
    r = hyrax_batch_check(vp, n, num_polys, num_points, d["queries"], d["proof"], hl.Hyrax.batch_verify,
                          hl.Keccak256Transcript.from_proof, mk)
    assert r.remaining() == 0
    bad = bytearray(d["proof"])
    bad[64 * num_polys * o_vp.num_chunks + 31] ^= 1  # the first evaluation
    with pytest.raises(hl.Error):
        hyrax_batch_check(vp, n, num_polys, num_points, d["queries"], bytes(bad), hl.Hyrax.batch_verify,
                          hl.Keccak256Transcript.from_proof, mk)
    # the last row commitment of poly 0 (it is absorbed before the batching challenges: the sum-check is the first to notice)
    swapped = _negate_point(d["proof"], 64 * (o_vp.num_chunks - 1))
    with pytest.raises(hl.Error):
        hyrax_batch_check(vp, n, num_polys, num_points, d["queries"], swapped, hl.Hyrax.batch_verify,
                          hl.Keccak256Transcript.from_proof, mk)


@pytest.mark.parametrize("n", range(1, 13))
def test_hyrax_setup_and_trim_dimensions(hl, n):
    """hyrax.rs:121-167: batch_num_vars = log2(next_pow2(poly_size batch_size)), row_num_vars = ceil(batch_num_vars / 2)"""
    poly_size = 1 << n
    for batch_size in sorted({1, 2, 3, poly_size}):
        if batch_size > poly_size:
            with pytest.raises(hl.ArgumentError):
                hl.Hyrax.dims(poly_size, batch_size)
            continue
        total = poly_size * batch_size
        bnv = next(k for k in range(64) if (1 << k) >= total)
        want = (n, bnv, -(-bnv // 2))
        assert hl.Hyrax.dims(poly_size, batch_size) == want == ir.hyrax_dims(poly_size, batch_size)
    if n <= 6:  # setup and trim themselves: the inner IPA has 2^row_num_vars generators; a smaller shape trims from it
        params = hl.Hyrax.setup(None, poly_size, poly_size)
        assert params.size == 1 << n  # batch_num_vars = 2 n
        vp = hl.Hyrax.trim(params, poly_size, 1)
        assert (vp.row_num_vars, vp.num_chunks) == (-(-n // 2), 1 << (n - -(-n // 2)))
        small = hl.Hyrax.setup(None, poly_size, 1)
        if n >= 2:
            with pytest.raises(hl.InvalidPcsParam, match="Too many variates to trim"):
                hl.Hyrax.trim(small, poly_size, poly_size)
            with pytest.raises(ir.PcsError, match="Too many variates to trim"):
                ir.hyrax_trim(ir.hyrax_setup(poly_size, 1), poly_size, poly_size)


def test_hyrax_asserts_and_null_arguments(hl):
    from halo2_lasso_amd import _ffi
    lib, out = _ffi.load(), C.c_void_p()
    assert lib.lh_hyrax_setup(None, 8, 0, C.byref(out)) == _ffi.LH_ERR_ARG   # 0 < batch_size (hyrax.rs:123)
    assert lib.lh_hyrax_setup(None, 8, 9, C.byref(out)) == _ffi.LH_ERR_ARG   # batch_size <= poly_size
    assert lib.lh_hyrax_setup(None, 6, 1, C.byref(out)) == _ffi.LH_ERR_ARG   # a power of two (hyrax.rs:122)
    params = hl.Hyrax.setup(None, 4, 1)
    g1, fr2, fr, ev = (_ffi.lh_g1 * 2)(), (_ffi.lh_fr * 2)(), _ffi.lh_fr(), (_ffi.lh_evaluation * 1)()
    t = hl.Keccak256Transcript.from_proof(b"")
    bad = [
        lib.lh_hyrax_setup(None, 4, 1, None),
        lib.lh_hyrax_trim(None, 4, 1, None, None),
        lib.lh_hyrax_verify(None, 4, 1, g1, fr2, 2, C.byref(fr), t.p),
        lib.lh_hyrax_verify(params.h, 4, 1, None, fr2, 2, C.byref(fr), t.p),
        lib.lh_hyrax_verify(params.h, 4, 1, g1, None, 2, C.byref(fr), t.p),
        lib.lh_hyrax_verify(params.h, 4, 1, g1, fr2, 2, None, t.p),
        lib.lh_hyrax_verify(params.h, 4, 1, g1, fr2, 2, C.byref(fr), None),
        lib.lh_hyrax_verify(params.h, 4, 1, g1, fr2, 1, C.byref(fr), t.p),  # a point of another length
        lib.lh_hyrax_batch_verify(None, 4, 1, 2, g1, 1, fr2, 1, ev, 1, t.p),
        lib.lh_hyrax_batch_verify(params.h, 4, 1, 2, None, 1, fr2, 1, ev, 1, t.p),
        lib.lh_hyrax_batch_verify(params.h, 4, 1, 2, g1, 1, None, 1, ev, 1, t.p),
        lib.lh_hyrax_batch_verify(params.h, 4, 1, 2, g1, 1, fr2, 1, None, 1, t.p),
        lib.lh_hyrax_batch_verify(params.h, 4, 1, 2, g1, 1, fr2, 1, ev, 1, None),
    ]
    assert bad == [_ffi.LH_ERR_ARG] * len(bad), bad


if __name__ == "__main__":
    gold = {"domain": ir.DOMAIN.decode(), "g": [[hex(c) for c in ir.generator_g(i)] for i in range(5)],
            "h": [hex(c) for c in ir.generator_h()]}
    with open(GOLDEN, "w") as f:
        json.dump(gold, f, indent=1)
        f.write("\n")
    print("wrote", GOLDEN)
