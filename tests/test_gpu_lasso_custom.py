"""GPU: Lasso into caller-registered subtables (hl.Subtable.register) - the gather kernel against numpy, proof bytes against
the Python oracle extended by tests/lasso_custom_ref.py over multilinear KZG (with the routes the commitments took, from the
launch records), a built-in table registered as a custom one at a size where the production routes run, HyperPlonk's Lasso
lookups, the column-committing schemes, and refusals that leave the ctx usable.

The named tables (lasso_custom_ref.TABLES): l = 3 and l = 4, where the derived route's window conditions hold from n = 1 on
(tests/test_gpu_lasso_tables.py test_derived_commitments_of_one_bit_subtables: pick_window floors the window at 4 and caps it at
the column's bits).  No sharded test: the worker of tests/test_gpu_sharded.py builds its tables by name in every rank's
process, and a registered table is a per-process registration.

Every test closes what it registers (tests/test_lasso_custom_cpu.py counts the live registrations).
"""
import array
import ctypes as C
import random

import numpy as np
import pytest

import lasso_custom_ref as lcr
import lasso_tables_ref as ltr
from oracle.pyref import kzg as o_kzg, lasso as o_lasso
from oracle.pyref.field import R_MOD as P
from oracle.pyref.transcript import Keccak256Transcript as OT

pytestmark = pytest.mark.gpu

KNOB = "LH_LASSO_PRODUCT_U32"
GATHER = "lasso_subtable_gather"


@pytest.fixture(scope="module")
def kzg6(hl, ctx):
    rng = random.Random(662)
    ss = [rng.randrange(1, P) for _ in range(6)]
    return o_kzg.setup(ss), hl.MultilinearKzg.setup(ctx, ss), hl.MultilinearKzgVerifierParams.setup(ss)


@pytest.fixture(scope="module")
def reg(hl):
    """name -> the registered Subtable of every named table, and of the LTU / EQ entries at l = 8"""
    values = dict(lcr.TABLES)
    values["ltu8"] = [ltr.ltu_entry(m, 8) for m in range(256)]
    values["eq8"] = [ltr.eq_entry(m, 8) for m in range(256)]
    tables = {name: hl.Subtable.register(v) for name, v in values.items()}
    yield tables
    for t in tables.values():
        t.close()


def _upload(ctx, dims):
    return [ctx.upload(array.array("I", d).tobytes()) for d in dims]


def _prove(hl, ctx, pp, table, n, dims):
    t = hl.Keccak256Transcript()
    hl.lasso_prove(pp, table, n, _upload(ctx, dims), t)
    return t.into_proof()


def _prove_profiled(hl, ctx, pp, table, n, dims):
    """-> (proof, the launch records)"""
    hl.profile_enable(ctx, True)
    try:
        proof = _prove(hl, ctx, pp, table, n, dims)
        return proof, hl.profile_read(ctx)
    finally:
        hl.profile_enable(ctx, False)


def _prove_all_routes(hl, ctx, monkeypatch, pp, table, n, dims):
    """one production prove and one with launch records - under both values of LH_LASSO_PRODUCT_U32 where g has a product term
    (tests/test_gpu_lasso_tables.py) - must give the same bytes -> (proof, the records of the last profiled prove)"""
    product = any(len(f) > 1 for _, f in table.g_terms)
    proofs, recs = [], None
    for value in ("0", "1") if product else (None,):
        if value is not None:
            monkeypatch.setenv(KNOB, value)
        proofs.append(_prove(hl, ctx, pp, table, n, dims))
        proof, recs = _prove_profiled(hl, ctx, pp, table, n, dims)
        proofs.append(proof)
        if product:
            names = [r["name"] for r in recs]
            assert names.count("lasso_output_small_prod") == (1 if value == "1" else 0), "switch at %s" % value
    if product:
        monkeypatch.delenv(KNOB)
    assert proofs[1:] == proofs[:-1], "the routes disagree"
    return proofs[0], recs


def _derived_items(recs):
    return sum(r["items"] for r in recs if r["name"] == "msm_derived")


# ------------------------------------------------------------------ 5. the gather kernel against numpy
GATHER_N = [1, 63, 64, 65, 255, 256, 257, 4097]
GATHER_L = [1, 3, 8, 14, 15, 16, 20]


@pytest.fixture(scope="module")
def gather_tables(hl):
    """l -> (Subtable, its values): random 32-bit values, 2^32 - 1 and 0 among them"""
    out = {}
    for l in GATHER_L:
        vals = np.random.default_rng(1000 + l).integers(0, 1 << 32, size=1 << l, dtype=np.uint64).astype(np.uint32)
        vals[0], vals[-1] = 0xFFFFFFFF, 0
        out[l] = (hl.Subtable.register(vals.tolist()), vals)
    yield out
    for t, _ in out.values():
        t.close()


def _gather_dims(l, n):
    """0, 2^l - 1 and a repeated index in every vector that has room for them (n = 1 holds one index: 2^l - 1)"""
    d = np.random.default_rng(7 * l + n).integers(0, 1 << l, size=n, dtype=np.uint64).astype(np.uint32)
    d[0] = (1 << l) - 1
    if n >= 4:
        d[1], d[2] = 0, d[3]
    return d


def _subtable_read(hl, ctx, kind, l, dims, offset=0):
    """lh_debug_lasso_subtable_read on columns that start `offset` entries into their buffers -> the n outputs; the entries
    around them must be left alone"""
    n = len(dims)
    d_in = ctx.upload(np.concatenate([np.zeros(offset, np.uint32), dims]).tobytes())
    guard = np.full(offset + n + 8, 0xA5A5A5A5, np.uint32)
    d_out = ctx.upload(guard.tobytes())
    rc = ctx.lib.lh_debug_lasso_subtable_read(ctx.h, int(kind), l, d_in.ptr + 4 * offset, n, d_out.ptr + 4 * offset)
    hl._check(rc)
    got = np.frombuffer(d_out.read(), dtype=np.uint32)
    assert (got[:offset] == 0xA5A5A5A5).all() and (got[offset + n:] == 0xA5A5A5A5).all(), "wrote outside its n entries"
    return got[offset:offset + n]


@pytest.mark.parametrize("l", GATHER_L)
@pytest.mark.parametrize("n", GATHER_N)
def test_gather_kernel_against_numpy(hl, ctx, gather_tables, n, l):
    t, vals = gather_tables[l]
    dims = _gather_dims(l, n)
    assert dims.max() == (1 << l) - 1 and (n < 4 or (dims.min() == 0 and dims[2] == dims[3]))
    want = vals[dims]
    assert (_subtable_read(hl, ctx, t, l, dims) == want).all()
    assert (_subtable_read(hl, ctx, t, l, dims, offset=1) == want).all()  # columns that are not 16-byte aligned
    # the mask: an index past the table reads T[index mod 2^l] (a prove refuses such a column; the kernel must not fault)
    far = dims.copy()
    far[0] |= np.uint32(1 << l) if l < 31 else 0
    far[-1] |= np.uint32(0x80000000)
    assert (_subtable_read(hl, ctx, t, l, far) == want).all()


def test_gather_of_registered_and_entries_is_the_builtin_read(hl, ctx, reg):
    for n in (1, 65, 4097):
        dims = _gather_dims(8, n)
        builtin = _subtable_read(hl, ctx, hl.SUBTABLE_AND, 8, dims)
        assert (builtin == ((dims >> 4) & (dims & 15))).all()
        assert (_subtable_read(hl, ctx, reg["and8"], 8, dims) == builtin).all()
    assert (_subtable_read(hl, ctx, hl.SUBTABLE_IDENTITY, 5, _gather_dims(5, 65)) == _gather_dims(5, 65)).all()
    for kind, l in ((6, 4), (reg["and8"].kind, 4), (reg["and8"].kind + 1000, 8), (hl.SUBTABLE_AND, 3)):
        d = ctx.upload(bytes(16))
        assert ctx.lib.lh_debug_lasso_subtable_read(ctx.h, kind, l, d.ptr, 4, d.ptr) == hl._ffi.LH_ERR_ARG


# ------------------------------------------------------------------ 6. proof bytes are the extended oracle's
BYTE_CASES = lcr.CASES + [("rand1", 2, 6, "linear")]  # (the CPU fixture's cases, and one with n > l)


@pytest.mark.parametrize("name,c,n,g", BYTE_CASES)
def test_proof_bytes_equal_the_oracle(hl, ctx, monkeypatch, kzg6, reg, name, c, n, g):
    opp, pp, vp = kzg6
    values, t = lcr.TABLES[name], reg[name]
    l = t.chunk_bits
    dims = lcr.random_dims(name, c, l, n)
    table = lcr.table_of(hl, name, c, g, t)
    with lcr.installed({t.kind: values}):
        ot = OT()
        o_lasso.prove(opp, lcr.spec_of(name, c, g, t.kind), dims, ot)
    proof, recs = _prove_all_routes(hl, ctx, monkeypatch, pp, table, n, dims)
    assert proof == ot.into_proof()
    tr = hl.Keccak256Transcript.from_proof(proof)
    hl.lasso_verify(vp, table, n, tr)
    assert tr.remaining() == 0
    names = [r["name"] for r in recs]
    assert names.count(GATHER) == c, "one gather per memory"
    asked = hl.lasso_last_route(ctx)["derived_commitments"]
    if name == "rand1":  # T[0] = 0: every E commitment from the buckets of its dim's
        assert asked == c and _derived_items(recs) == c * (1 << l)
    elif name == "rand1n":  # T[0] = 1: ordinary 32-bit columns
        assert asked == 0 and "msm_derived" not in names
    elif name == "wide":  # bytes only; the route is recorded (32-bit values fail the derived job's window condition)
        print("wide: derived asked %d, gathered %d" % (asked, _derived_items(recs)))
    elif name == "zero":  # a = E = 0: identity commitments under the mask
        assert int.from_bytes(proof[:32], "big") != 0


def test_less_than_signed_proof_bytes_equal_the_oracle(hl, ctx, monkeypatch, kzg6):
    opp, pp, vp = kzg6
    c, l, n = 2, 4, 5
    table = hl.LassoTable.less_than_signed(c, l)
    top = table.memories[c - 1][1]
    dims = lcr.comparison_dims(c, l, n)
    with lcr.installed({top.kind: lcr.lts_values(l)}):
        ot = OT()
        o_lasso.prove(opp, lcr.less_than_signed_spec(c, l, top.kind), dims, ot)
    proof, recs = _prove_all_routes(hl, ctx, monkeypatch, pp, table, n, dims)
    assert proof == ot.into_proof()
    hl.lasso_verify(vp, table, n, hl.Keccak256Transcript.from_proof(proof))
    # LTU of chunk 0 and the signed subtable derive (T[0] = 0), EQ does not
    assert hl.lasso_last_route(ctx)["derived_commitments"] == 2 and _derived_items(recs) == 2 * (1 << l)
    assert [r["name"] for r in recs].count(GATHER) == 1


# ------------------------------------------------------------------ 7. at a size where the production routes run
@pytest.fixture(scope="module")
def kzg14(hl, ctx):
    rng = random.Random(1414)
    ss = [rng.randrange(1, P) for _ in range(14)]
    return hl.MultilinearKzg.setup(ctx, ss), hl.MultilinearKzgVerifierParams.setup(ss)


@pytest.mark.parametrize("which", ["and", "less_than"])
def test_a_builtin_registered_as_custom_gives_the_builtin_proof(hl, ctx, kzg14, reg, which):
    pp, vp = kzg14
    n, c, l = 14, 2, 8
    if which == "and":
        builtin = hl.LassoTable.bitwise(hl.SUBTABLE_AND, c, l)
        swap = {hl.SUBTABLE_AND: reg["and8"]}
    else:
        builtin = hl.LassoTable.less_than(c, l)
        swap = {hl.SUBTABLE_LTU: reg["ltu8"], hl.SUBTABLE_EQ: reg["eq8"]}  # (registered EQ has T[0] = 1: an ordinary column)
    custom = hl.LassoTable(c, l, [(j, swap[kind]) for j, kind in builtin.memories], builtin.g_terms)
    dims = [np.random.default_rng(140 + j).integers(0, 1 << l, size=1 << n, dtype=np.uint32) for j in range(c)]
    if which == "less_than":
        for d in dims:  # equal halves in a third of the lookups
            d[::3] = (d[::3] >> 4) * 17
    want = _prove(hl, ctx, pp, builtin, n, dims)
    derived = hl.lasso_last_route(ctx)["derived_commitments"]
    got, recs = _prove_profiled(hl, ctx, pp, custom, n, dims)
    assert got == want
    assert _prove(hl, ctx, pp, custom, n, dims) == want  # (and without the records' synchronisation)
    assert hl.lasso_last_route(ctx)["derived_commitments"] == derived == 2
    assert [r["name"] for r in recs].count(GATHER) == len(custom.memories)
    for table in (builtin, custom):
        tr = hl.Keccak256Transcript.from_proof(got)
        hl.lasso_verify(vp, table, n, tr)
        assert tr.remaining() == 0


# ------------------------------------------------------------------ 8. HyperPlonk's Lasso lookups
def test_hyperplonk_with_a_registered_subtable(hl, ctx, reg):
    from halo2_lasso_amd import hyperplonk as g_hp
    from oracle.pyref import hyperplonk as o_hp
    num_vars, c = 5, 2
    t = reg["rand1"]
    spec, table = lcr.spec_of("rand1", c, "linear", t.kind), lcr.table_of(hl, "rand1", c, "linear", t)
    rng = random.Random(505)
    ss = [rng.randrange(1, P) for _ in range(num_vars)]
    with lcr.installed({t.kind: lcr.TABLES["rand1"]}):
        from oracle.pyref.transcript import TranscriptError
        for seed in range(58, 66):  # (a witness column that is identically zero commits to the identity, which HyperPlonk's
            o_info, instances, witness = o_hp.rand_vanilla_plonk_with_lasso_circuit(num_vars, random.Random(seed), spec)
            o_pp = o_hp.preprocess(o_kzg.setup(ss), o_info)  # transcript cannot encode: the next seed then, as make_golden.py)
            ot = OT()
            try:
                o_hp.prove(o_pp, instances, lambda r, ch: witness, ot)
                break
            except TranscriptError:
                continue
        want = ot.into_proof()
        assert any(witness[3 + c]), "some lookup reads a one"
        o_hp.verify(o_pp, instances, OT(want))
    g_info = g_hp.vanilla_plonk_with_lasso_circuit_info(num_vars, len(instances[0]), o_info.preprocess_polys,
                                                        o_info.permutations, table)
    g_pp, g_vp = g_hp.HyperPlonk.preprocess(hl.MultilinearKzg.setup(ctx, ss), g_info, hl.MultilinearKzgVerifierParams.setup(ss))
    tr = hl.Keccak256Transcript()
    g_hp.HyperPlonk.prove(g_pp, instances, [hl.MultilinearPolynomial.new(ctx, x) for x in witness], tr)
    proof = tr.into_proof()
    assert proof == want
    r = hl.Keccak256Transcript.from_proof(proof)
    g_hp.HyperPlonk.verify(g_vp, instances, r)
    assert r.remaining() == 0
    # a chunk value outside the subtable is the reference's error, as under a built-in kind
    bad = [list(x) for x in witness]
    bad[3][2] = 1 << t.chunk_bits
    with pytest.raises(hl.InvalidSnark, match="Invalid lookup input"):
        g_hp.HyperPlonk.prove(g_pp, instances, [hl.MultilinearPolynomial.new(ctx, x) for x in bad], hl.Keccak256Transcript())


# ------------------------------------------------------------------ 9. the column-committing schemes
@pytest.mark.parametrize("scheme", ["hyrax", "zeromorph", "brakedown"])
def test_column_committing_schemes_prove_and_verify(hl, ctx, monkeypatch, reg, scheme):
    """the independent host verifier is the yardstick (the argument's bytes: the KZG tests above)"""
    if scheme == "brakedown":  # the shape of tests/brakedown_lasso_ref.py case "a" with rand1 in place of the range table
        import brakedown_lasso_ref as bl
        name, c, n, g = "rand1", 2, 4, "linear"
        assert bl.CASES["a"][1:4] == (c, lcr.bits_of(lcr.TABLES[name]), n)
    else:
        name, c, n, g = "rand1n", 2, 2, "product"
    t = reg[name]
    l = t.chunk_bits
    nv = max(n, l)
    if scheme == "hyrax":
        pp = hl.Hyrax.trim(hl.Hyrax.setup(ctx, 1 << nv, 1), 1 << nv, 1)
        vps = [hl.Hyrax.trim(hl.Hyrax.setup(None, 1 << nv, 1), 1 << nv, 1)]
    elif scheme == "zeromorph":
        s = 0x5eed + 12
        pp = hl.Zeromorph.trim(hl.Zeromorph.setup(ctx, s, 1 << nv), 1 << nv)
        vps = [hl.ZeromorphVerifierParam.setup(s, 1 << nv, 1 << nv)]
    else:
        pp = hl.Brakedown.setup(ctx, nv, bl.SPEC, bl.SEED)
        vps = [pp, hl.BrakedownVerifierParam.setup(nv, bl.SPEC, bl.SEED)]
    table = lcr.table_of(hl, name, c, g, t)
    dims = lcr.random_dims(name, c, l, n)
    proof, recs = _prove_all_routes(hl, ctx, monkeypatch, pp, table, n, dims)
    assert [r["name"] for r in recs].count(GATHER) == c
    for vp in vps:
        tr = hl.Keccak256Transcript.from_proof(proof)
        hl.lasso_verify(vp, table, n, tr)
        assert tr.remaining() == 0
    bad = bytearray(proof)
    bad[len(bad) // 2] ^= 8
    with pytest.raises(hl.Error):
        hl.lasso_verify(vps[-1], table, n, hl.Keccak256Transcript.from_proof(bytes(bad)))
    with hl.Subtable.register([1 - v for v in lcr.TABLES[name]]) as other:  # the same proof under another table
        with pytest.raises(hl.Error):
            hl.lasso_verify(vps[-1], lcr.table_of(hl, name, c, g, other), n, hl.Keccak256Transcript.from_proof(proof))


# ------------------------------------------------------------------ 10. refusals leave the ctx usable
def test_refusals_leave_the_ctx_usable(hl, ctx, kzg6, reg):
    _, pp, vp = kzg6
    n, l = 5, 4
    good = lcr.random_dims("wide", 1, l, n)
    bad = [list(good[0])]
    bad[0][17] = 1 << l  # not an index of the 2^l-entry subtable

    def status(table, dims):
        try:
            _prove(hl, ctx, pp, table, n, dims)
        except hl.Error as e:
            return e.code
        return 0
    custom = lcr.table_of(hl, "wide", 1, "linear", reg["wide"])
    # the same status as under a built-in kind, and no device error: the gather masked the index
    refused = status(custom, bad)
    assert refused == status(hl.LassoTable.bitwise(hl.SUBTABLE_AND, 1, l), bad)
    assert refused not in (0, hl._ffi.LH_ERR_DEVICE)
    assert status(custom, good) == 0
    # a stale kind and a chunk_bits mismatch, past the Python side's own check: the library's
    d_dims = _upload(ctx, good)
    gone = hl.Subtable.register(lcr.TABLES["wide"])
    stale = lcr.table_of(hl, "wide", 1, "linear", gone).to_c()
    gone.close()
    mismatch = custom.to_c()
    mismatch.chunk_bits = l + 1
    for tc in (stale, mismatch):
        t = hl.Keccak256Transcript()
        assert ctx.lib.lh_lasso_prove(ctx.h, pp.h, C.byref(tc), n, hl._ptr_array(d_dims), t.p) == hl._ffi.LH_ERR_ARG
    with pytest.raises(hl.ArgumentError):
        hl.lasso_prove(pp, hl.LassoTable(1, l + 1, custom.memories, custom.g_terms), n, d_dims, hl.Keccak256Transcript())
    # then a good proof on the same ctx
    proof = _prove(hl, ctx, pp, custom, n, good)
    hl.lasso_verify(vp, custom, n, hl.Keccak256Transcript.from_proof(proof))
