"""GPU: HyperPlonk over MultilinearBrakedown (lh_hyperplonk_prove[_phases]_brakedown: Pcs::commit_and_write over the batched
commit, the batch opening over the staged matrix) against the oracle's proofs as recorded in
tests/golden/brakedown_hyperplonk.json (length, SHA-256, preprocess and permutation roots: the proofs are 8 and 36 MB),
through lh_hyperplonk_verify[_phases]_brakedown with a host-only and with the device param; the batched commit against single
commits and the restatement; the staged matrix against the transpose of the rows and the staged open against the column
round trips; the refusals, and that a refused or failed prove leaves nothing behind.

What the sizes put under test:
  num_vars 3, Spec6    one row, a codeword of 14 (depth 4): no proximity rows, no staging launch, a tile with 14 of 16 columns
  num_vars 12, Spec6   case (b): the first size with more than one row - 2 rows of 2048, a codeword of 3523 (220 full tiles and
                       one of 3 columns, 2 of 16 rows)
  num_vars 14, Spec6   the first size with 4 rows: 4 of 16 tile rows, a codeword of 7046 (440 full tiles and one of 6 columns)
"""
import ctypes as C
import hashlib
import random

import numpy as np
import pytest

import brakedown_provers_ref as bp
import brakedown_ref as br

pytestmark = pytest.mark.gpu

P = br.P
TILE = 16  # kernels_brakedown.hip BD_T


# ------------------------------------------------------------------ shared state, made once
_params, _proved = {}, {}


def _pp(hl, ctx, num_vars, spec):
    if (num_vars, spec) not in _params:
        _params[(num_vars, spec)] = hl.Brakedown.setup(ctx, num_vars, spec, bp.SEED)
    return _params[(num_vars, spec)]


def _g_info(case, o_info, instances):
    from halo2_lasso_amd import hyperplonk as g_hp
    mk = g_hp.vanilla_plonk_with_lookup_circuit_info if case[2] else g_hp.vanilla_plonk_circuit_info
    info = mk(case[0], len(instances[0]), o_info.preprocess_polys, o_info.permutations)
    info.num_witness_polys, info.num_challenges = list(case[3]), [0] * len(case[3])
    return info


def _prove(hl, ctx, name):
    """-> (case, instances, prover param, verifier param over the device param, proof) of a fixture case, proved once"""
    if name not in _proved:
        from halo2_lasso_amd import hyperplonk as g_hp
        case = bp.cases()[name]
        o_info, instances, witness_fn = bp.circuit(case)
        pcs = _pp(hl, ctx, case[0], case[1])
        g_pp, g_vp = g_hp.HyperPlonk.preprocess(pcs, _g_info(case, o_info, instances), pcs)
        calls = []

        def synth(rnd, challenges):
            calls.append(rnd)
            return [hl.MultilinearPolynomial.new(ctx, w) for w in witness_fn(rnd, challenges)]
        t = hl.Keccak256Transcript()
        g_hp.HyperPlonk.prove(g_pp, instances, synth if len(case[3]) > 1 else synth(0, []), t)
        assert calls == list(range(len(case[3])))
        _proved[name] = (case, instances, g_pp, g_vp, t.into_proof())
    return _proved[name]


def _open_bytes(p):
    rows = (p.num_proximity_testing + 1) * p.row_len if p.num_rows > 1 else p.row_len
    return 32 * (rows + p.num_column_opening * (p.num_rows + p.depth))


# ------------------------------------------------------------------ 1. proof bytes
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_proof_is_the_oracles_and_verifies(hl, ctx, name):
    from halo2_lasso_amd import hyperplonk as g_hp
    fx = bp.fixture()[name]
    case, instances, g_pp, g_vp, proof = _prove(hl, ctx, name)
    print("case %s: %d bytes, sha256 %s" % (name, len(proof), hashlib.sha256(proof).hexdigest()))
    assert [c.root.hex() for c in g_pp.preprocess_comms] == fx["preprocess_roots"]
    assert [c.root.hex() for c in g_pp.permutation_comms] == fx["permutation_roots"]
    assert g_vp.preprocess_comms == [c.root for c in g_pp.preprocess_comms]
    assert len(proof) == fx["proof_len"]
    assert hashlib.sha256(proof).hexdigest() == fx["proof_sha256"]
    # both verifier params: the device one, and a host-only one (a verifier without a GPU)
    host_vp = g_hp.HyperPlonkVerifierParam()
    host_vp.__dict__.update(g_vp.__dict__)
    host_vp.pcs = hl.BrakedownVerifierParam.setup(case[0], case[1], bp.SEED)
    for vp in (g_vp, host_vp):
        r = hl.Keccak256Transcript.from_proof(proof)
        g_hp.HyperPlonk.verify(vp, instances, r)
        assert r.remaining() == 0
    # the proof ends in num_evaluations field elements and as many openings; field elements travel most significant byte first
    p = br.Params(case[0], case[1])
    ne, one = fx["num_evaluations"], _open_bytes(p)
    evals_at = len(proof) - ne * one - 32 * ne
    assert evals_at > 0
    bad = bytearray(proof)
    bad[evals_at + 31] ^= 1  # the first written evaluation
    with pytest.raises(hl.InvalidSnark):
        g_hp.HyperPlonk.verify(host_vp, instances, hl.Keccak256Transcript.from_proof(bytes(bad)))
    rows = (p.num_proximity_testing + 1) * p.row_len if p.num_rows > 1 else p.row_len
    bad = bytearray(proof)
    bad[evals_at + 32 * ne + 32 * rows + 31] ^= 1  # the first entry of the first opened column of the first opening
    with pytest.raises(hl.InvalidPcsOpen, match="^(Proximity failure|Invalid merkle tree opening)$"):
        g_hp.HyperPlonk.verify(host_vp, instances, hl.Keccak256Transcript.from_proof(bytes(bad)))
    wrong = g_hp.HyperPlonkVerifierParam()
    wrong.__dict__.update(host_vp.__dict__)
    wrong.preprocess_comms = [bytes([host_vp.preprocess_comms[0][0] ^ 1]) + host_vp.preprocess_comms[0][1:]] + \
        list(host_vp.preprocess_comms[1:])
    with pytest.raises(hl.InvalidPcsOpen, match="^Invalid merkle tree opening$"):
        g_hp.HyperPlonk.verify(wrong, instances, hl.Keccak256Transcript.from_proof(proof))


# ------------------------------------------------------------------ 2. batched commit
def _rand_polys(ctx, hl, num_vars, count, seed):
    rng = random.Random(seed)
    tabs = [[rng.randrange(P) for _ in range(1 << num_vars)] for _ in range(count)]
    return tabs, [hl.MultilinearPolynomial.new(ctx, t) for t in tabs]


@pytest.mark.parametrize("num_vars", [3, 12])
def test_batched_commit_equals_single_commits(hl, ctx, num_vars):
    nv_b, spec = bp.cases()["b"][:2]
    assert num_vars in (3, nv_b)
    pp = _pp(hl, ctx, num_vars, spec)
    o_pp = br.Params(num_vars, spec, bp.SEED) if num_vars <= 6 else None
    tabs, polys = _rand_polys(ctx, hl, num_vars, 3, 40 + num_vars)
    tabs.append([0] * (1 << num_vars))
    polys.append(hl.MultilinearPolynomial.new(ctx, tabs[-1]))
    single = [hl.Brakedown.commit(pp, p) for p in polys]  # (lh_brakedown_commit: its own kernels)
    assert hl.get_option(ctx, "brakedown_batch_commit") == 1
    for batch in ([0], [0, 1, 2], [3], [1, 3, 0, 2]):  # P = 1, P = 3, the all-zero poly alone and inside a batch
        comms = hl.Brakedown.batch_commit(pp, [polys[i] for i in batch])
        for i, c in zip(batch, comms):
            assert c.root == single[i].root
            assert c.tree(pp.codeword_len) == single[i].tree(pp.codeword_len)
            assert c.tree(pp.codeword_len)[-32:] == c.root
            assert c.rows(pp.num_rows, pp.codeword_len) == single[i].rows(pp.num_rows, pp.codeword_len)
    if o_pp is not None:
        for i, tab in enumerate(tabs):
            want = br.commit(o_pp, tab)
            assert single[i].root == want.root and single[i].tree(pp.codeword_len) == b"".join(want.hashes)
            assert comms[batch.index(i)].rows(pp.num_rows, pp.codeword_len) == [x for row in want.rows for x in row]
    # the literal route (a commit per poly) is still there and agrees
    try:
        hl.set_option(ctx, "brakedown_batch_commit", 0)
        assert [c.root for c in hl.Brakedown.batch_commit(pp, polys)] == [c.root for c in single]
    finally:
        hl.set_option(ctx, "brakedown_batch_commit", 1)


# ------------------------------------------------------------------ 3. staged open
def _odd_size():
    """a size whose codeword_len and num_rows are no multiples of the tile (and with more than one tile of columns)"""
    for nv in range(13, 20):
        p = br.Params(nv, 6)
        if p.num_rows % TILE and p.codeword_len % TILE and p.num_rows >= 4:
            return nv
    raise AssertionError("no such size")


@pytest.mark.parametrize("which", ["one-row", "case-b", "odd"])
def test_staged_matrix_and_staged_open(hl, ctx, which):
    num_vars = {"one-row": 3, "case-b": bp.cases()["b"][0], "odd": _odd_size()}[which]
    pp = _pp(hl, ctx, num_vars, 6)
    R, cw = pp.num_rows, pp.codeword_len
    if which == "one-row":
        assert (R, cw) == (1, 14)
    elif which == "odd":
        assert R % TILE and cw % TILE
    _, polys = _rand_polys(ctx, hl, num_vars, 1, 90 + num_vars)
    poly = polys[0]
    comm = hl.Brakedown.commit(pp, poly)
    raw = C.create_string_buffer(32 * R * cw)
    hl._check(ctx.lib.lh_brakedown_comm_rows(ctx.h, comm.h, raw))
    rows = np.frombuffer(raw.raw, dtype=np.uint8).reshape(R, cw, 32)
    staged = np.frombuffer(comm.staged(pp), dtype=np.uint8).reshape(cw, R, 32)
    assert np.array_equal(staged, rows.transpose(1, 0, 2))
    rng = random.Random(5)
    points = [[rng.randrange(P) for _ in range(num_vars)] for _ in range(2)]
    evals = [hl.Evaluation(0, k, hl.evaluate_polys(ctx, [poly], pt)[0]) for k, pt in enumerate(points)]
    t0 = hl.Keccak256Transcript()
    for pt in points:  # the column round trips: two lh_brakedown_open calls
        hl.Brakedown.open(pp, poly, comm, pt, t0)
    want = t0.into_proof()
    assert hl.get_option(ctx, "brakedown_staged_open") == 0
    try:
        hl.set_option(ctx, "brakedown_staged_open", 1)
        t1 = hl.Keccak256Transcript()
        hl.Brakedown.batch_open(pp, num_vars, [poly], [comm], points, evals, t1)
    finally:
        hl.set_option(ctx, "brakedown_staged_open", 0)
    got = t1.into_proof()
    assert len(got) == 2 * _open_bytes(br.Params(num_vars, 6)) and got == want
    r = hl.Keccak256Transcript.from_proof(got)
    hl.Brakedown.batch_verify(pp, num_vars, [comm.root], points, evals, r)
    assert r.remaining() == 0


# ------------------------------------------------------------------ 4. refusals
def test_refusals_and_that_nothing_is_left_behind(hl, ctx):
    from halo2_lasso_amd import _ffi, hyperplonk as g_hp
    case, instances, g_pp, g_vp, _ = _prove(hl, ctx, "c")
    _, _, witness_fn = bp.circuit(case)
    lib = ctx.lib

    # a Lasso lookup in the circuit: refused before anything is committed
    lasso_info = g_hp.PlonkishCircuitInfo.__new__(g_hp.PlonkishCircuitInfo)
    lasso_info.__dict__.update(g_pp.info.__dict__)
    lasso_info.lasso_lookups = [g_hp.LassoLookup(hl.LassoTable.range(1, 4), 12, [11])]
    with_lasso = g_hp.HyperPlonkProverParam()
    with_lasso.__dict__.update(g_pp.__dict__)
    with_lasso.info = lasso_info
    synth = lambda rnd, ch: [hl.MultilinearPolynomial.new(ctx, w) for w in witness_fn(rnd, ch)]
    with pytest.raises(hl.ArgumentError, match="Lasso lookups"):
        g_hp.HyperPlonk.prove(with_lasso, instances, synth, hl.Keccak256Transcript())

    # a circuit of another size than the param's
    small = g_hp.HyperPlonkProverParam()
    small.__dict__.update(g_pp.__dict__)
    small.num_vars = case[0] - 1
    with pytest.raises(hl.ArgumentError, match="variables"):
        g_hp.HyperPlonk.prove(small, instances, synth, hl.Keccak256Transcript())

    # NULL arguments of the entries
    t = hl.Keccak256Transcript()
    hio = C.byref(t.hash_io())
    prm = _ffi.lh_hp_param()
    prm.num_vars, prm.num_witness_polys = case[0], 1
    circ = _ffi.lh_hp_circuit()
    wit = (C.c_void_p * 1)(g_pp.preprocess_polys[0].ptr)
    h, p = ctx.h, g_pp.pcs.h
    bad = [lib.lh_hyperplonk_prove_brakedown(None, p, C.byref(prm), None, None, None, wit, t.p, hio),
           lib.lh_hyperplonk_prove_brakedown(h, None, C.byref(prm), None, None, None, wit, t.p, hio),
           lib.lh_hyperplonk_prove_brakedown(h, p, None, None, None, None, wit, t.p, hio),
           lib.lh_hyperplonk_prove_brakedown(h, p, C.byref(prm), None, None, None, None, t.p, hio),
           lib.lh_hyperplonk_prove_brakedown(h, p, C.byref(prm), None, None, None, wit, None, hio),
           lib.lh_hyperplonk_prove_brakedown(h, p, C.byref(prm), None, None, None, wit, t.p, None),
           lib.lh_hyperplonk_prove_phases_brakedown(None, p, C.byref(prm), None, None, 0, None, None, None, C.byref(circ), t.p, hio),
           lib.lh_hyperplonk_prove_phases_brakedown(h, None, C.byref(prm), None, None, 0, None, None, None, C.byref(circ), t.p, hio),
           lib.lh_hyperplonk_prove_phases_brakedown(h, p, None, None, None, 0, None, None, None, C.byref(circ), t.p, hio),
           lib.lh_hyperplonk_prove_phases_brakedown(h, p, C.byref(prm), None, None, 0, None, None, None, None, t.p, hio)]
    prm.num_preprocess_polys = 1  # commitments may be NULL only when there are none
    bad.append(lib.lh_hyperplonk_prove_brakedown(h, p, C.byref(prm), None, None, None, wit, t.p, hio))
    assert b"preprocess_comms" in lib.lh_last_error()
    assert bad == [_ffi.LH_ERR_ARG] * len(bad), bad

    # a prove that fails after its first commit round (the second phase's synthesize gives up), and a refused one: ten
    # repeats hold no more memory than one
    class GiveUp(Exception):
        pass

    def failing(rnd, ch):
        if rnd == 1:
            raise GiveUp()
        return synth(rnd, ch)

    def once():
        with pytest.raises(GiveUp):
            g_hp.HyperPlonk.prove(g_pp, instances, failing, hl.Keccak256Transcript())
        with pytest.raises(hl.ArgumentError):
            g_hp.HyperPlonk.prove(small, instances, synth, hl.Keccak256Transcript())
    once()
    before = hl.memory_stats(ctx)
    for _ in range(10):
        once()
    after = hl.memory_stats(ctx)
    assert after["arena_reserved_bytes"] == before["arena_reserved_bytes"]
    assert after["arena_high_water_bytes"] == before["arena_high_water_bytes"]
    assert after["device_free_bytes"] >= before["device_free_bytes"] - (1 << 20)
    # ... and the ctx still proves the same bytes
    t = hl.Keccak256Transcript()
    g_hp.HyperPlonk.prove(g_pp, instances, synth, t)
    assert hashlib.sha256(t.into_proof()).hexdigest() == bp.fixture()["c"]["proof_sha256"]
