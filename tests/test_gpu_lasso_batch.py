"""GPU: lookups into several tables in one proof (hl.lasso_prove_batch) - proof bytes against the golden proofs of the
reference (tests/lasso_batch_ref.py, tests/golden/lasso_batch.json), the host verifier, the launch records of the shared-column
route, the route switches, every table's commitment block against its own lasso_prove proof, a size at which the streaming
kernels run (n = 13, no Python reference: the verifier, the switches and the single-table proofs are the check), refusals."""
import array
import ctypes as C
import json
import os
import random

import pytest

import lasso_batch_ref as lbr
from oracle.pyref.field import R_MOD as P

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "lasso_batch.json")))["cases"]
SS = [int(x, 16) for x in json.load(open(os.path.join(HERE, "golden", "lasso_tables.json")))["srs"]["ss"]]
SWITCHES = ["gkr_resident", "sc_tail", "sc_eq_factoring", "lasso_pack_ts"]
KNOB = "LH_LASSO_PRODUCT_U32"


@pytest.fixture(scope="module")
def kzg6(hl, ctx):
    assert len(SS) == 6
    return hl.MultilinearKzg.setup(ctx, SS), hl.MultilinearKzgVerifierParams.setup(SS)


def _upload(ctx, dims):
    return [ctx.upload(array.array("I", d).tobytes()) for d in dims]


def _case(hl, ctx, case, kind=None):
    """-> (tables, n, device columns per table); a SHARED case hands every table the first table's buffers"""
    n, descs = lbr.CASES[case]
    tables = [lbr.table_of(hl, d, kind) for d in descs]
    dims = GOLDEN[case]["dims"]
    cols = [_upload(ctx, d) for d in dims]
    return tables, n, cols * len(tables) if case in lbr.SHARED else cols


def _prove(hl, pp, tables, n, cols):
    t = hl.Keccak256Transcript()
    hl.lasso_prove_batch(pp, tables, n, cols, t)
    return t.into_proof()


def _prove_single(hl, pp, table, n, cols):
    t = hl.Keccak256Transcript()
    hl.lasso_prove(pp, table, n, cols, t)
    return t.into_proof()


def _profiled(hl, ctx, fn):
    hl.profile_enable(ctx, True)
    try:
        out = fn()
        return out, hl.profile_read(ctx)
    finally:
        hl.profile_enable(ctx, False)


def _block_bytes(stream, count):
    """bytes of the commitment block that starts `stream`: the mask element, then 64 per commitment that is not the identity"""
    mask = int.from_bytes(stream[:32], "little")
    assert mask >> count == 0
    return 32 + 64 * (count - bin(mask).count("1"))


def _check_blocks(hl, pp, tables, n, cols, proof):
    at = 0
    for table, c in zip(tables, cols):
        single = _prove_single(hl, pp, table, n, c)
        size = _block_bytes(single, 1 + 3 * table.c + len(table.memories))
        assert proof[at:at + size] == single[:size]
        at += size


class _registered:
    def __init__(self, hl, case):
        values = list(lbr.custom_values(case).values())
        self.t = hl.Subtable.register(values[0]) if values else None

    def __enter__(self):
        return self.t

    def __exit__(self, *exc):
        if self.t is not None:
            self.t.close()


# ------------------------------------------------------------------ 1. bytes and the verifier
@pytest.mark.parametrize("case", list(lbr.CASES))
def test_proof_bytes_equal_the_golden_and_verify(hl, ctx, kzg6, case):
    pp, vp = kzg6
    with _registered(hl, case) as kind:
        tables, n, cols = _case(hl, ctx, case, kind)
        proof = _prove(hl, pp, tables, n, cols)
        assert proof.hex() == GOLDEN[case]["proof"]
        t = hl.Keccak256Transcript.from_proof(proof)
        hl.lasso_verify_batch(vp, tables, n, t)
        assert t.remaining() == 0
    if case == "zeros":  # identity commitments under both masks
        assert int.from_bytes(proof[:32], "little") != 0


# ------------------------------------------------------------------ 2. launch records of the shared-column route
def _commit_reduces(recs, leaf):
    names = [r["name"] for r in recs]
    return names[:names.index(leaf)].count("msm_bucket_reduce")


def test_shared_columns_are_counted_and_committed_once(hl, ctx, kzg6):
    pp, _ = kzg6
    tables, n, cols = _case(hl, ctx, "and_xor_shared")
    assert cols[0] is cols[1] or [a.ptr for a in cols[0]] == [b.ptr for b in cols[1]]
    proof, recs = _profiled(hl, ctx, lambda: _prove(hl, pp, tables, n, cols))
    assert proof.hex() == GOLDEN["and_xor_shared"]["proof"]
    names = [r["name"] for r in recs]
    assert names.count("lasso_rw_leaves_batch") == 1 and "lasso_rw_leaves" not in names
    counters = [r for r in recs if r["name"] == "lasso_counters"]
    assert len(counters) == 1 and counters[0]["items"] == 2 << n, "two shared columns, counted once"
    # one commit batch for the proof: what ONE single-table prove launches, not twice that
    _, single = _profiled(hl, ctx, lambda: _prove_single(hl, pp, tables[0], n, cols[0]))
    assert _commit_reduces(recs, "lasso_rw_leaves_batch") == _commit_reduces(single, "lasso_rw_leaves") >= 1
    # distinct buffers with the same contents: the same bytes, both tables counted
    copies = [_upload(ctx, GOLDEN["and_xor_shared"]["dims"][0]) for _ in tables]
    proof2, recs2 = _profiled(hl, ctx, lambda: _prove(hl, pp, tables, n, copies))
    assert proof2 == proof and [r["name"] for r in recs2].count("lasso_counters") == 2


# ------------------------------------------------------------------ 3. route switches
def _switched(hl, ctx, fn):
    """fn() with every switch of SWITCHES at 0, one at a time"""
    out = []
    for name in SWITCHES:
        before = hl.get_option(ctx, name)
        hl.set_option(ctx, name, 0)
        try:
            out.append(fn())
        finally:
            hl.set_option(ctx, name, before)
    return out


def test_route_switches_keep_the_bytes(hl, ctx, kzg6, monkeypatch):
    pp, _ = kzg6
    tables, n, cols = _case(hl, ctx, "two_ranges")
    for proof in _switched(hl, ctx, lambda: _prove(hl, pp, tables, n, cols)):
        assert proof.hex() == GOLDEN["two_ranges"]["proof"]
    tables, n, cols = _case(hl, ctx, "mixed_g")
    for value in ("0", "1"):
        monkeypatch.setenv(KNOB, value)
        proof, recs = _profiled(hl, ctx, lambda: _prove(hl, pp, tables, n, cols))
        assert proof.hex() == GOLDEN["mixed_g"]["proof"], "switch at %s" % value
        assert [r["name"] for r in recs].count("lasso_output_small_prod") == int(value)
    monkeypatch.delenv(KNOB)


# ------------------------------------------------------------------ 4. a table's block is the block of its own proof
@pytest.mark.parametrize("case", ["two_ranges", "full"])
def test_commitment_blocks_equal_the_single_proofs(hl, ctx, kzg6, case):
    pp, _ = kzg6
    tables, n, cols = _case(hl, ctx, case)
    assert all(max(n, t.l) == max([n] + [u.l for u in tables]) for t in tables), "the single proofs commit at the batch's nv"
    _check_blocks(hl, pp, tables, n, cols, bytes.fromhex(GOLDEN[case]["proof"]))


# ------------------------------------------------------------------ 5. n = 13: fused leaves, launched tree levels, derived commitments
def test_n13(hl, ctx):
    n, l = 13, 8
    rng = random.Random(1313)
    ss = [rng.randrange(1, P) for _ in range(n)]
    pp, vp = hl.MultilinearKzg.setup(ctx, ss), hl.MultilinearKzgVerifierParams.setup(ss)
    tables = [hl.LassoTable.range(2, l), hl.LassoTable.bitwise(hl.SUBTABLE_XOR, 2, l)]
    import numpy as np
    gen = np.random.default_rng(13)
    cols = [[ctx.upload(gen.integers(0, 1 << l, size=1 << n, dtype=np.uint32).tobytes()) for _ in range(2)] for _ in tables]
    proof, recs = _profiled(hl, ctx, lambda: _prove(hl, pp, tables, n, cols))
    names = [r["name"] for r in recs]
    assert names.count("lasso_rw_leaves_batch") == 1 and "tree_up" in names
    assert _prove(hl, pp, tables, n, cols) == proof
    route = hl.lasso_last_route(ctx)
    assert route["derived_commitments"] >= 1 and route["resident_layers"] >= 1
    timing = hl.lasso_last_timing(ctx)
    assert timing["total"] > 0 and all(timing[k] >= 0 for k in ("witness", "commit", "surge", "leaves", "gkr", "evals", "open_n"))
    t = hl.Keccak256Transcript.from_proof(proof)
    hl.lasso_verify_batch(vp, tables, n, t)
    assert t.remaining() == 0
    bad = bytearray(proof)
    bad[len(bad) // 2] ^= 1
    with pytest.raises(hl.InvalidSnark):
        hl.lasso_verify_batch(vp, tables, n, hl.Keccak256Transcript.from_proof(bytes(bad)))
    for other in _switched(hl, ctx, lambda: _prove(hl, pp, tables, n, cols)):
        assert other == proof
    _check_blocks(hl, pp, tables, n, cols, proof)
    pp.free()


# ------------------------------------------------------------------ 6. refusals
def test_refusals_leave_the_ctx_usable(hl, ctx, kzg6):
    pp, vp = kzg6
    tables, n, cols = _case(hl, ctx, "two_ranges")
    hl.attach_comm(ctx, 0, 2, lambda send: send * 2, 1)  # a ctx of a sharded world
    try:
        with pytest.raises(hl.ArgumentError, match="sharded"):
            _prove(hl, pp, tables, n, cols)
    finally:
        hl.detach_comm(ctx)
    # the sum of the memories: less_than(4, 4) has 7, range(2, 2) has 2
    lt = hl.LassoTable.less_than(4, 4)
    zeros = _upload(ctx, [[0] * (1 << n)] * 4)
    with pytest.raises(hl.ArgumentError, match="memories"):
        _prove(hl, pp, [lt, tables[0]], n, [zeros, cols[0]])
    # an index >= 2^l in one table's column: as from the single prover
    dims = [list(d) for d in GOLDEN["two_ranges"]["dims"][1]]
    dims[1][5] = 1 << tables[1].l
    with pytest.raises(hl.ArgumentError, match="out of range"):
        _prove(hl, pp, tables, n, [cols[0], _upload(ctx, dims)])
    with pytest.raises(hl.ArgumentError, match="out of range"):
        _prove_single(hl, pp, tables[1], n, _upload(ctx, dims))
    # NULL lists and columns straight through ctypes
    t = hl.Keccak256Transcript()
    one = tables[0].to_c()
    arr = (C.POINTER(hl._ffi.lh_lasso_table) * 1)(C.pointer(one))
    holed = (C.POINTER(C.c_void_p) * 1)(C.cast(hl._ptr_array([cols[0][0], None]), C.POINTER(C.c_void_p)))
    lib = ctx.lib
    assert lib.lh_lasso_prove_batch(ctx.h, pp.h, arr, 1, n, None, t.p) == hl._ffi.LH_ERR_ARG
    assert lib.lh_lasso_prove_batch(ctx.h, pp.h, None, 1, n, holed, t.p) == hl._ffi.LH_ERR_ARG
    assert lib.lh_lasso_prove_batch(ctx.h, pp.h, arr, 1, n, holed, t.p) == hl._ffi.LH_ERR_ARG
    assert lib.lh_lasso_prove_batch(ctx.h, None, arr, 1, n, holed, t.p) == hl._ffi.LH_ERR_ARG
    assert len(t.into_proof()) == 0
    # max(n, max l) above the SRS
    with pytest.raises(hl.InvalidPcsParam):
        _prove(hl, pp, [tables[0], hl.LassoTable.range(1, 7)], n, [cols[0], _upload(ctx, [[0] * (1 << n)])])
    # the ctx proves `single` afterwards
    tables, n, cols = _case(hl, ctx, "single")
    proof = _prove(hl, pp, tables, n, cols)
    assert proof.hex() == GOLDEN["single"]["proof"]
    hl.lasso_verify_batch(vp, tables, n, hl.Keccak256Transcript.from_proof(proof))
