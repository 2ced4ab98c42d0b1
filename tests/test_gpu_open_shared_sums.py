"""The batch opening takes the quad sums that the argument's evaluation passes made at the same points (csrc/sumcheck.cpp
quad_sums_*, csrc/lasso.cpp; LH_OPEN_SHARE_SUMS, default 1) instead of summing the columns again.  2^22 lookups is the
smallest size at which the opening's sum-check takes its first rounds from the columns.

The switch changes who makes the sums, never the bytes: proofs with it on and off are identical and verify; the route
counter open_shared_sums says how many (column, point) pairs the opening found in the proof's table; the profile of the
opening shows a quad-sum launch for the short final_cts columns at most.  The table is keyed by device pointers that the arena
hands out again proof after proof: two proofs over different lookups back to back on one ctx must each equal the proof of a
fresh ctx.  And since the evaluations written to the transcript now come from the four sums through a host identity, a flipped
lookup index must change the proof and leave it valid.

The number of n-variable (column, point) pairs of a table with c chunks and alpha memories: the output column a at r (ONE
column: the opening's term at r carries a itself, not its expansion into the E columns), the alpha E columns at r_z, and
dim | read_ts | E = 2 c + alpha columns at r_N: 1 + alpha + 2 c + alpha.  For the AND table (c = alpha = 4) that is 17, for the
range check (c = alpha = 2; E of the identity subtable IS the dim column, the pair is looked up under both names) 9."""
import os
import random

import numpy as np
import pytest

from oracle.pyref.field import R_MOD as P

pytestmark = pytest.mark.gpu

N = 22
KNOB = "LH_OPEN_SHARE_SUMS"


def make_table(hl, kind):
    return hl.LassoTable.range(2, 16) if kind == "range" else hl.LassoTable.bitwise(hl.SUBTABLE_AND, 4, 16)


def pairs_of(table):
    c, alpha = table.c, len(table.memories)
    return 1 + alpha + (2 * c + alpha)


def make_dims(table, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 1 << table.l, size=1 << N, dtype=np.uint32) for _ in range(table.c)]


@pytest.fixture(scope="module")
def srs(hl, ctx):
    rng = random.Random(2207)
    ss = [rng.randrange(1, P) for _ in range(N)]
    return ss, hl.MultilinearKzg.setup(ctx, ss), hl.MultilinearKzgVerifierParams.setup(ss)


def prove(hl, ctx, pp, table, dims, share=None, profile=False):
    """-> (proof bytes, route, profile records); share: the switch's value for this prove (None: unset, the default)"""
    before = os.environ.pop(KNOB, None)
    if share is not None:
        os.environ[KNOB] = str(share)
    recs = []
    try:
        t = hl.Keccak256Transcript()
        bufs = [ctx.upload(d.tobytes()) for d in dims]
        if profile:
            hl.profile_enable(ctx, True)
        try:
            hl.lasso_prove(pp, table, N, bufs, t)
            if profile:
                recs = hl.profile_read(ctx)
        finally:
            if profile:
                hl.profile_enable(ctx, False)
        return t.into_proof(), hl.lasso_last_route(ctx), recs
    finally:
        os.environ.pop(KNOB, None)
        if before is not None:
            os.environ[KNOB] = before


@pytest.fixture(scope="module")
def and_proof(hl, ctx, srs):
    """one AND proof with the default route, shared by the tests below: (table, dims, proof)"""
    table = make_table(hl, "and")
    dims = make_dims(table, 2201)
    return table, dims, prove(hl, ctx, srs[1], table, dims)[0]


@pytest.mark.parametrize("kind", ["and", "range"])
def test_switch_changes_who_sums_not_the_bytes(hl, ctx, srs, kind):
    ss, pp, vp = srs
    table = make_table(hl, kind)
    dims = make_dims(table, 2201 if kind == "and" else 2202)
    on, route_on, recs_on = prove(hl, ctx, pp, table, dims, share=1, profile=True)
    off, route_off, recs_off = prove(hl, ctx, pp, table, dims, share=0, profile=True)
    assert on == off
    hl.lasso_verify(vp, table, N, hl.Keccak256Transcript.from_proof(on))
    assert route_off["open_shared_sums"] == 0, route_off
    assert route_on["open_shared_sums"] == pairs_of(table), (route_on, pairs_of(table))
    # profile records come in launch order.  Off: no quad_sums pass anywhere; Surge's round 0 and the opening's four terms
    # launch inner_products<quads>.  On: the evaluations at r_z and r_N are quad_sums passes, and behind the last of them - the
    # opening - inner_products<quads> appears for the term of the c final_cts columns at r_M at most
    names_on, names_off = [r["name"] for r in recs_on], [r["name"] for r in recs_off]
    assert "quad_sums" not in names_off and names_off.count("inner_products<quads>") == 1 + 4, names_off
    assert names_on.count("quad_sums") == 2, names_on
    last = len(names_on) - 1 - names_on[::-1].index("quad_sums")
    opening = [r for r in recs_on[last + 1:] if r["name"] == "inner_products<quads>"]
    assert len(opening) <= 1 and names_on[:last].count("inner_products<quads>") == 1, names_on
    quads = 1 << (N - 2)
    for r in opening:  # (k_inner_products_quads books 16 B per column quad and the eq table once per pair of columns)
        assert r["items"] == quads and r["bytes"] == 16.0 * quads * table.c + 32.0 * quads * ((table.c + 1) // 2), (r, table.c)


def test_default_is_on(hl, ctx, srs, and_proof):
    table, dims, proof = and_proof
    again, route, _ = prove(hl, ctx, srs[1], table, dims)
    assert again == proof and route["open_shared_sums"] == pairs_of(table), route


def test_back_to_back_proofs_do_not_see_each_others_sums(hl, ctx, srs, and_proof):
    """same sizes, so the same arena pointers: a stale entry of the first proof would answer the second one's lookups"""
    ss, pp, vp = srs
    table, dims_a, _ = and_proof
    dims_b = make_dims(table, 2203)
    a, route_a, _ = prove(hl, ctx, pp, table, dims_a)
    b, route_b, _ = prove(hl, ctx, pp, table, dims_b)
    assert a != b and route_a["open_shared_sums"] == route_b["open_shared_sums"] == pairs_of(table)
    for dims, proof in ((dims_a, a), (dims_b, b)):
        fresh = hl.Context(0)
        try:
            assert prove(hl, fresh, hl.MultilinearKzg.setup(fresh, ss), table, dims)[0] == proof
        finally:
            fresh.close()
    hl.lasso_verify(vp, table, N, hl.Keccak256Transcript.from_proof(b))


def test_flipped_lookup_changes_the_proof_and_it_still_verifies(hl, ctx, srs, and_proof):
    ss, pp, vp = srs
    table, dims, proof = and_proof
    flipped = [d.copy() for d in dims]
    flipped[1][(1 << N) - 5] ^= 1
    other, route, _ = prove(hl, ctx, pp, table, flipped)
    assert other != proof and route["open_shared_sums"] == pairs_of(table), route
    hl.lasso_verify(vp, table, N, hl.Keccak256Transcript.from_proof(other))
