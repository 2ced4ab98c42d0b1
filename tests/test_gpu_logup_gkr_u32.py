"""GPU: LogUp-GKR from 32-bit input columns (hl.U32Column, lh_logup_gkr_prove_columns).  A u32 column and the same values
as field elements are the same polynomial, so every proof is compared with the golden bytes of the unchanged specification
(tests/golden/logup_gkr_u32.json) AND with the bytes of the existing entry on the widened columns; then the route switches
(the column-wise opening among them), the launch records of the mixed-column compression, a size with many workgroups in
every kernel, refusals."""
import array
import importlib.util
import json
import os
import random

import pytest

import logup_gkr_ref as lgr
from oracle.pyref.field import R_MOD as P

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_logup_gkr_u32", os.path.join(HERE, "golden", "make_logup_gkr_u32.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)
GOLDEN = json.load(open(os.path.join(HERE, "golden", "logup_gkr_u32.json")))["cases"]
SS = [int(x, 16) for x in json.load(open(os.path.join(HERE, "golden", "lasso_tables.json")))["srs"]["ss"]]
SWITCHES = ["logup_fused_leaves", "gkr_resident", "sc_tail", "sc_eq_factoring"]
LARGE = (16, 10, [[1, 1]])


@pytest.fixture(scope="module")
def kzg6(hl, ctx):
    assert len(SS) == 6
    return hl.MultilinearKzg.setup(ctx, SS), hl.MultilinearKzgVerifierParams.setup(SS)


@pytest.fixture(scope="module")
def kzg16(hl, ctx):
    """the recipe of test_gpu_logup_gkr.py: sixteen variables whose first fourteen secrets are `mid`'s"""
    rng = random.Random(lgr.MID_SRS_SEED + 1)
    ss = lgr.mid_ss() + [rng.randrange(1, P) for _ in range(2)]
    return hl.MultilinearKzg.setup(ctx, ss), hl.MultilinearKzgVerifierParams.setup(ss)


def _column(hl, ctx, col, kind):
    if kind:
        return hl.U32Column(ctx.upload(array.array("I", col).tobytes()), len(col).bit_length() - 1)
    return hl.MultilinearPolynomial.new(ctx, col)


def _lookups(hl, ctx, tables, rows, kinds):
    """kinds None: every column as field elements (the existing entry)"""
    ins = lgr.inputs_of(tables, rows)
    return [hl.LogupLookup([_column(hl, ctx, col, ks[j] if ks else 0) for j, col in enumerate(f)], t)
            for f, t, ks in zip(ins, tables, kinds or [None] * len(tables))]


_made = {}


def _case(hl, ctx, case, u32=True):
    """the case's lookups, uploaded once and shared (nothing writes to them)"""
    if (case, u32) not in _made:
        _made[case, u32] = _lookups(hl, ctx, gen.case_tables(case), GOLDEN[case]["rows"], gen.CASES[case][2] if u32 else None)
    return _made[case, u32]


def _prove(hl, pp, lookups):
    t = hl.Keccak256Transcript()
    hl.logup_gkr_prove(pp, lookups, t)
    return t.into_proof()


def _profiled(hl, ctx, fn):
    hl.profile_enable(ctx, True)
    try:
        out = fn()
        return out, hl.profile_read(ctx)
    finally:
        hl.profile_enable(ctx, False)


class _option:
    def __init__(self, hl, ctx, name, value):
        self.hl, self.ctx, self.name, self.value = hl, ctx, name, value

    def __enter__(self):
        self.old = self.hl.get_option(self.ctx, self.name)
        self.hl.set_option(self.ctx, self.name, self.value)

    def __exit__(self, *exc):
        self.hl.set_option(self.ctx, self.name, self.old)


# ------------------------------------------------------------------ 1. bytes: the golden ones, the Fr entry's, the verifier
@pytest.mark.parametrize("case", list(gen.CASES))
def test_proof_bytes_equal_the_golden_and_the_fr_entrys(hl, ctx, kzg6, kzg16, case):
    pp, vp = kzg6 if case in gen.SMALL else kzg16
    lookups = _case(hl, ctx, case)
    assert [[isinstance(p, hl.U32Column) for p in lk.inputs] for lk in lookups] == [[bool(k) for k in ks] for ks in gen.CASES[case][2]]
    proof = _prove(hl, pp, lookups)
    assert proof.hex() == GOLDEN[case]["proof"]
    assert _prove(hl, pp, _case(hl, ctx, case, u32=False)) == proof, "the existing entry on the widened columns"
    t = hl.Keccak256Transcript.from_proof(proof)
    hl.logup_gkr_verify(vp, [hl.LogupLookup(None, lk.table) for lk in lookups], gen.CASES[case][0], t)
    assert t.remaining() == 0
    if case == "u32_zeros":  # the all-zero u32 column commits to the identity: bit 0 of the first mask
        assert int.from_bytes(proof[:32], "big") == 1


# ------------------------------------------------------------------ 2. the route switches: same bytes
@pytest.mark.parametrize("case", ["u32_mixed", "u32_mid"])
def test_bytes_do_not_depend_on_the_switches(hl, ctx, kzg6, kzg16, case):
    pp, _ = kzg6 if case in gen.SMALL else kzg16
    lookups = _case(hl, ctx, case)
    for name in SWITCHES:
        with _option(hl, ctx, name, 0):
            assert _prove(hl, pp, lookups).hex() == GOLDEN[case]["proof"], name + " = 0"
    if case == "u32_mid":
        # every opened poly is a 32-bit column: from open_small_min_vars on the opening commits its largest quotients
        # column by column.  13 variables are below the default; with the threshold lowered the route is taken
        assert _prove(hl, pp, lookups).hex() == GOLDEN[case]["proof"]
        assert hl.lasso_last_route(ctx)["open_small_depth"] == 0
        with _option(hl, ctx, "open_small_min_vars", 8):
            assert _prove(hl, pp, lookups).hex() == GOLDEN[case]["proof"], "the column-wise opening"
            assert hl.lasso_last_route(ctx)["open_small_depth"] >= 1, "the column route was not taken"


# ------------------------------------------------------------------ 3. launch records
def test_launch_records_of_the_compression(hl, ctx, kzg6, kzg16):
    pp, _ = kzg16
    case = "u32_mid"
    n, l, kinds = gen.CASES[case]
    widths = [len(ks) for ks in kinds]
    proof, recs = _profiled(hl, ctx, lambda: _prove(hl, pp, _case(hl, ctx, case)))
    assert proof.hex() == GOLDEN[case]["proof"]
    cols = [r for r in recs if r["name"] == "logup_compress_cols"]
    # one per lookup (a single u32 column is widened by it): 4 B per u32 entry read, 32 B per row written
    assert [(r["items"], r["bytes"]) for r in cols] == [(1 << n, (4 * w + 32) << n) for w in widths]
    # the input side of an all-u32 lookup launches no logup_compress; the table side of a tuple still does
    assert [r["items"] for r in recs if r["name"] == "logup_compress"] == [1 << l] * sum(w > 1 for w in widths)
    assert [r["items"] for r in recs if r["name"] == "logup_m"] == [1 << n] * len(widths)
    # a mixed lookup: 4 or 32 bytes per column entry
    n5, l5, kinds5 = gen.CASES["u32_mixed"]
    _, recs = _profiled(hl, ctx, lambda: _prove(hl, kzg6[0], _case(hl, ctx, "u32_mixed")))
    assert [(r["items"], r["bytes"]) for r in recs if r["name"] == "logup_compress_cols"] == \
        [(1 << n5, (sum(4 if k else 32 for k in kinds5[0]) + 32) << n5)]
    assert [r["items"] for r in recs if r["name"] == "logup_compress"] == [1 << l5], "lookup 1 is a single Fr column"
    # an all-Fr proof still records what it recorded
    proof_fr, recs = _profiled(hl, ctx, lambda: _prove(hl, pp, _case(hl, ctx, case, u32=False)))
    assert proof_fr == proof
    names = [r["name"] for r in recs]
    assert "logup_compress_cols" not in names and names.count("logup_compress") == 2 * sum(w > 1 for w in widths)
    assert [r["items"] for r in recs if r["name"] == "logup_compress"] == [1 << n, 1 << l]


# ------------------------------------------------------------------ 4. a size with many workgroups in every kernel
def test_larger_shape_equals_the_fr_proof_and_verifies(hl, ctx, kzg16):
    pp, vp = kzg16
    n, l, kinds = LARGE
    rng = random.Random(1611)
    tables = [[[rng.randrange(1 << 32) for _ in range(1 << l)] for _ in ks] for ks in kinds]
    rows = [[rng.randrange(1 << l) for _ in range(1 << n)] for _ in kinds]
    proof = _prove(hl, pp, _lookups(hl, ctx, tables, rows, kinds))
    assert proof == _prove(hl, pp, _lookups(hl, ctx, tables, rows, None))
    t = hl.Keccak256Transcript.from_proof(proof)
    hl.logup_gkr_verify(vp, [hl.LogupLookup(None, tb) for tb in tables], n, t)
    assert t.remaining() == 0


# ------------------------------------------------------------------ 5. refusals, and the ctx afterwards
def test_refusals_and_the_ctx_goes_on(hl, ctx, kzg6):
    from halo2_lasso_amd import _ffi
    pp, _ = kzg6
    lib = ctx.lib
    one_var = lambda: _prove(hl, pp, _case(hl, ctx, "u32_one_var")).hex() == GOLDEN["u32_one_var"]["proof"]
    n = gen.CASES["u32_mixed"][0]
    # kind 2
    arr, table_vars, keep = hl._logup_list(_case(hl, ctx, "u32_mixed"), n, True, True)
    arr[0].kinds[2] = 2
    t = hl.Keccak256Transcript()
    assert lib.lh_logup_gkr_prove_columns(ctx.h, pp.h, arr, 2, n, table_vars, t.p) == _ffi.LH_ERR_ARG
    msg = lib.lh_last_error()
    assert b"lookup 0" in msg and b"column 2" in msg and b"kind" in msg and not t.into_proof(), "refused before a byte is written"
    assert one_var()
    # a null u32 column
    arr, table_vars, keep = hl._logup_list(_case(hl, ctx, "u32_mixed"), n, True, True)
    arr[0].d_inputs[0] = None
    t = hl.Keccak256Transcript()
    assert lib.lh_logup_gkr_prove_columns(ctx.h, pp.h, arr, 2, n, table_vars, t.p) == _ffi.LH_ERR_ARG
    assert b"input column" in lib.lh_last_error() and not t.into_proof()
    assert one_var()
    # NULL kinds: every column an Fr column - the existing entry's bytes
    arr, table_vars, keep = hl._logup_list(_case(hl, ctx, "u32_mixed", u32=False), n, True, True)
    for k in range(2):
        arr[k].kinds = None
    t = hl.Keccak256Transcript()
    assert lib.lh_logup_gkr_prove_columns(ctx.h, pp.h, arr, 2, n, table_vars, t.p) == _ffi.LH_OK
    assert t.into_proof().hex() == GOLDEN["u32_mixed"]["proof"]
    # a u32 input that is in no table row
    for case, k, j in (("u32_edges", 0, 0), ("u32_mixed", 0, 2)):
        tables = gen.case_tables(case)
        ins = lgr.inputs_of(tables, GOLDEN[case]["rows"])
        ins[k][j][-1] = next(v for v in range(2, 1000) if v not in tables[k][j])
        kinds = gen.CASES[case][2]
        lookups = [hl.LogupLookup([_column(hl, ctx, col, ks[i]) for i, col in enumerate(f)], tb)
                   for f, tb, ks in zip(ins, tables, kinds)]
        with pytest.raises(hl.InvalidSnark, match="Invalid lookup input"):
            hl.logup_gkr_prove(pp, lookups, hl.Keccak256Transcript())
        assert one_var()
