"""The opening's precommit in two stages (option open_precommit_stages, csrc/open_columns.cpp): the helper ctx queues the
column differences, the digits and the sort of the entries behind the commit batch's bucket accumulation (stage 1) and
its own accumulation only where the product trees are built (stage 2), behind a host-side gate.  The staging moves work
in time, never a byte: every comparison here is on proof bytes, against the C++ oracle (oracle/cpu) where one proof of
it serves several tests.

2^17 range lookups is the smallest proof whose opening takes the column route (two dim and two read_ts columns:
column_route_on), so the smallest with a precommit at all; 2^21 AND lookups is the smallest AND proof that takes it - packed
pairs and eight jobs, so stage 1 has real sorts.  The AND case compares the two settings with each other on the sample
bench.py proves at that size: the oracle's 2^21 AND proof takes ~10 s, and tests/test_gpu_parity_large.py already pins the
default route at that size to the oracle (test_lasso_default_route_at_2p21_matches_cpp_oracle).

The gate can be left closed by nothing: the knob LH_TEST_PRECOMMIT_GATE (a test hook) makes the trees' callback a no-op, so
that the plan is released only when the opening takes it (1), or is cancelled by the opening, which then commits the
column-wise levels itself (2); a transcript that fails on the first challenge after the commitments cancels a plan whose
first stage is in flight and whose gate is closed.  Nothing here waits for a time limit: every path ends on the host."""
import ctypes as C
import os
import random

import numpy as np
import pytest

from oracle import cpu_oracle as co
from oracle.pyref.field import R_MOD as P

pytestmark = pytest.mark.gpu

N = 17
GATE = "LH_TEST_PRECOMMIT_GATE"


@pytest.fixture(scope="module")
def srs(hl, ctx):
    rng = random.Random(1719)
    ss = [rng.randrange(1, P) for _ in range(N)]
    pp = hl.MultilinearKzg.setup(ctx, ss)
    return ss, pp, pp.eqs_bytes()


@pytest.fixture(scope="module")
def sample(hl, srs):
    """(table, columns, the oracle's proof) of the 2^17 range check every test below proves"""
    table = hl.LassoTable.range(2, 16)
    rng = np.random.default_rng(1720)
    dims = [rng.integers(0, 1 << table.l, size=1 << N, dtype=np.uint32) for _ in range(table.c)]
    ot = co.Transcript()
    co.lasso_prove(ot, srs[2], N, table.to_c(), N, [d.tobytes() for d in dims])
    return table, dims, ot.into_proof()


def fresh_ctx(hl, srs):
    """a ctx of its own over the module's SRS (options are per ctx; the SRS stays the fixture's)"""
    c = hl.Context(0)
    return c, hl.MultilinearKzgParams(c, srs[1].h)


def prove(hl, c, pp, table, dims, n=N, transcript=None):
    t = transcript or hl.Keccak256Transcript()
    hl.lasso_prove(pp, table, n, [c.upload(d.tobytes()) for d in dims], t)
    return (t.into_proof() if transcript is None else None), hl.lasso_last_route(c)


class gate:
    """LH_TEST_PRECOMMIT_GATE for the duration of a block (the knob is read at every use)"""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.before = os.environ.get(GATE)
        os.environ[GATE] = str(self.value)

    def __exit__(self, *exc):
        os.environ.pop(GATE, None)
        if self.before is not None:
            os.environ[GATE] = self.before


def test_two_stages_and_one_give_the_oracles_bytes(hl, srs, sample):
    table, dims, want = sample
    c, pp = fresh_ctx(hl, srs)
    try:
        assert hl.get_option(c, "open_precommit_stages") in (0, 1)
        for stages in (1, 0):
            hl.set_option(c, "open_precommit_stages", stages)
            proof, route = prove(hl, c, pp, table, dims)
            assert proof == want, stages
            assert route["open_precommit"] == 1 and route["open_precommit_staged"] == stages, (stages, route)
        with pytest.raises(hl.Error):
            hl.set_option(c, "open_precommit_stages", 2)
    finally:
        pp.h = None
        c.close()


def test_two_staged_proofs_back_to_back(hl, srs, sample):
    """the second proof's stage 1 starts on a helper that holds nothing of the first; other lookups, so other bytes"""
    table, dims, want = sample
    other = [d[::-1].copy() for d in dims]
    c, pp = fresh_ctx(hl, srs)
    c2, pp2 = fresh_ctx(hl, srs)
    try:
        hl.set_option(c, "open_precommit_stages", 1)
        hl.set_option(c2, "open_precommit_stages", 1)
        first, route_a = prove(hl, c, pp, table, dims)
        second, route_b = prove(hl, c, pp, table, other)
        assert first == want and second != first
        assert route_a["open_precommit_staged"] == route_b["open_precommit_staged"] == 1
        assert route_a["open_precommit"] == route_b["open_precommit"] == 1
        assert prove(hl, c2, pp2, table, other)[0] == second
    finally:
        pp.h = pp2.h = None
        c.close()
        c2.close()


def test_and_2p21_staged_equals_single_stage(hl, ctx):
    """packed pairs, eight jobs: the sizes at which stage 1 sorts 2^20-point slabs; bench.py's sample of that size"""
    from halo2_lasso_amd import dist as hdist
    n = 21
    table = hl.LassoTable.bitwise(hl.SUBTABLE_AND, 4, 16)
    rng = np.random.Generator(np.random.PCG64(hdist.batch_seed(n, 0)))
    dims = [rng.integers(0, 1 << table.l, size=1 << n, dtype=np.uint32) for _ in range(table.c)]
    trap = random.Random(2119)
    ss = [trap.randrange(1, P) for _ in range(n)]
    c = hl.Context(0)
    try:
        pp = hl.MultilinearKzg.setup(c, ss)
        proofs = {}
        for stages in (1, 0):
            hl.set_option(c, "open_precommit_stages", stages)
            proofs[stages], route = prove(hl, c, pp, table, dims, n)
            assert route["open_precommit"] == 1 and route["open_precommit_staged"] == stages, (stages, route)
            assert route["open_small_passes"] >= 3, route
        assert proofs[1] == proofs[0]
        hl.lasso_verify(hl.MultilinearKzgVerifierParams.setup(ss), table, n, hl.Keccak256Transcript.from_proof(proofs[1]))
    finally:
        c.close()


def test_stage_2_released_only_by_the_opening(hl, srs, sample):
    """nothing happens where the trees are built: the opening's take opens the gate, and still gets the precommit"""
    table, dims, want = sample
    c, pp = fresh_ctx(hl, srs)
    try:
        hl.set_option(c, "open_precommit_stages", 1)
        with gate(1):
            proof, route = prove(hl, c, pp, table, dims)
        assert proof == want and route["open_precommit"] == 1 and route["open_precommit_staged"] == 1, route
        proof, route = prove(hl, c, pp, table, dims)  # (and the ctx goes on as usual)
        assert proof == want and route["open_precommit"] == 1 and route["open_precommit_staged"] == 1, route
    finally:
        pp.h = None
        c.close()


def test_opening_declines_a_staged_precommit(hl, srs, sample):
    """the plan is cancelled with its gate closed (stage 2 never runs) and the opening commits the column-wise levels itself"""
    table, dims, want = sample
    c, pp = fresh_ctx(hl, srs)
    try:
        hl.set_option(c, "open_precommit_stages", 1)
        with gate(2):
            proof, route = prove(hl, c, pp, table, dims)
        assert proof == want and route["open_precommit_staged"] == 1, route
        assert route["open_precommit"] == 0 and route["open_small_depth"] >= 1 and route["open_small_passes"] >= 1, route
        proof, route = prove(hl, c, pp, table, dims)
        assert proof == want and route["open_precommit"] == 1, route
    finally:
        pp.h = None
        c.close()


def test_prove_that_fails_after_stage_1(hl, srs, sample):
    """the transcript fails on the first challenge after the commitments: stage 1 is in flight, the gate closed.  The error is
    the transcript's, and the next proof on the ctx has the oracle's bytes."""
    from halo2_lasso_amd import _ffi
    table, dims, want = sample
    c, pp = fresh_ctx(hl, srs)
    try:
        hl.set_option(c, "open_precommit_stages", 1)
        inner = hl.Keccak256Transcript()
        vt = inner.p.contents
        calls = {"n": 0}

        def squeeze(user, out):
            calls["n"] += 1
            return -6  # LH_ERR_TRANSCRIPT

        failing = _ffi.lh_transcript()
        C.memmove(C.byref(failing), inner.p, C.sizeof(failing))
        cb = _ffi._FE_CB(squeeze)
        failing.squeeze_challenge = cb

        class Wrapped:
            p = C.pointer(failing)

        with pytest.raises(hl.TranscriptError):
            prove(hl, c, pp, table, dims, transcript=Wrapped)
        assert calls["n"] == 1
        assert hl.lasso_last_route(c)["open_precommit_staged"] == 1  # (the commit batch had started it)
        proof, route = prove(hl, c, pp, table, dims)
        assert proof == want and route["open_precommit"] == 1 and route["open_precommit_staged"] == 1, route
    finally:
        pp.h = None
        c.close()
