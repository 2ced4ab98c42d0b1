"""GPU: the LogUp-GKR lookup argument (hl.logup_gkr_prove) - proof bytes against the golden proofs of the specification
(tests/logup_gkr_ref.py, tests/golden/logup_gkr.json), the host verifier, the route switches, the launch records of the
fused leaf kernel, the multiplicities read back through the proof, a size at which every kernel runs many workgroups
(n = 16, no Python reference: the verifier and the switch are the check), refusals."""
import json
import os
import random

import pytest

import logup_gkr_ref as lgr
from oracle.pyref.field import R_MOD as P
from oracle.pyref.poly import evaluate

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "logup_gkr.json")))["cases"]
SS = [int(x, 16) for x in json.load(open(os.path.join(HERE, "golden", "lasso_tables.json")))["srs"]["ss"]]
SWITCHES = ["logup_fused_leaves", "gkr_resident", "sc_tail", "sc_eq_factoring"]
LARGE = (16, 10, [1])


@pytest.fixture(scope="module")
def kzg6(hl, ctx):
    assert len(SS) == 6
    return hl.MultilinearKzg.setup(ctx, SS), hl.MultilinearKzgVerifierParams.setup(SS)


@pytest.fixture(scope="module")
def kzg16(hl, ctx):
    """sixteen variables whose first fourteen secrets are `mid`'s: a level depends on the secrets below it alone"""
    rng = random.Random(lgr.MID_SRS_SEED + 1)
    ss = lgr.mid_ss() + [rng.randrange(1, P) for _ in range(2)]
    return hl.MultilinearKzg.setup(ctx, ss), hl.MultilinearKzgVerifierParams.setup(ss)


def _lookups(hl, ctx, tables, rows):
    ins = lgr.inputs_of(tables, rows)
    return [hl.LogupLookup([hl.MultilinearPolynomial.new(ctx, col) for col in f], t) for f, t in zip(ins, tables)]


def _case(hl, ctx, case):
    return _lookups(hl, ctx, lgr.case_tables(case), GOLDEN[case]["rows"])


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


# ------------------------------------------------------------------ 1. bytes and the verifier
@pytest.mark.parametrize("case", list(lgr.CASES))
def test_proof_bytes_equal_the_golden_and_verify(hl, ctx, kzg6, kzg16, case):
    pp, vp = kzg6 if case in lgr.SMALL else kzg16
    lookups = _case(hl, ctx, case)
    proof = _prove(hl, pp, lookups)
    assert proof.hex() == GOLDEN[case]["proof"]
    t = hl.Keccak256Transcript.from_proof(proof)
    hl.logup_gkr_verify(vp, lookups, lgr.CASES[case][0], t)
    assert t.remaining() == 0
    if case == "zeros":  # the all-zero input column commits to the identity: bit 0 of the first mask (its repr is big-endian)
        assert int.from_bytes(proof[:32], "big") == 1


# ------------------------------------------------------------------ 2. the route switches: same bytes
@pytest.mark.parametrize("case", ["small_table", "big_table", "mid"])
def test_bytes_do_not_depend_on_the_switches(hl, ctx, kzg6, kzg16, case):
    pp, _ = kzg6 if case in lgr.SMALL else kzg16
    lookups = _case(hl, ctx, case)
    assert hl.get_option(ctx, "logup_fused_leaves") in (0, 1)
    for name in SWITCHES:
        with _option(hl, ctx, name, 0):
            assert _prove(hl, pp, lookups).hex() == GOLDEN[case]["proof"], name + " = 0"
    with _option(hl, ctx, "logup_fused_leaves", 1):
        assert _prove(hl, pp, lookups).hex() == GOLDEN[case]["proof"]


# ------------------------------------------------------------------ 3. launch records
@pytest.mark.parametrize("case", ["small_table", "mid"])
def test_launch_records_of_the_leaf_kernels(hl, ctx, kzg6, kzg16, case):
    pp, _ = kzg6 if case in lgr.SMALL else kzg16
    n, l, widths = lgr.CASES[case]
    L = len(widths)
    lookups = _case(hl, ctx, case)
    with _option(hl, ctx, "logup_fused_leaves", 1):
        proof, recs = _profiled(hl, ctx, lambda: _prove(hl, pp, lookups))
    assert proof.hex() == GOLDEN[case]["proof"]
    names = [r["name"] for r in recs]
    fused = [r for r in recs if r["name"] == "logup_leaves_up"]
    assert [r["items"] for r in fused] == [L << (n - 1), L << (l - 1)], "once per side: the inputs', then the table's"
    assert "logup_leaves" not in names
    # every layer above the fused one still comes from frac_up: (n - 2) + (l - 2) levels of L fractions
    assert names.count("frac_up") == L * ((n - 2) + (l - 2))
    # a tuple is compressed in one launch per side, a single column in none; one join per lookup over its 2^n inputs
    assert names.count("logup_compress") == 2 * sum(w > 1 for w in widths)
    assert [r["items"] for r in recs if r["name"] == "logup_m"] == [1 << n] * L
    with _option(hl, ctx, "logup_fused_leaves", 0):
        proof, recs = _profiled(hl, ctx, lambda: _prove(hl, pp, lookups))
    assert proof.hex() == GOLDEN[case]["proof"]
    names = [r["name"] for r in recs]
    assert "logup_leaves_up" not in names
    assert [r["items"] for r in recs if r["name"] == "logup_leaves"] == [L << (n - 1), L << (l - 1)]
    assert names.count("frac_up") == L * ((n - 1) + (l - 1))


# ------------------------------------------------------------------ 4. the multiplicities, read back through the proof
def _claims(hl, proof, n, l, widths):
    """the verifier's walk over a proof with the package's own transcript: -> (x_l, the evaluations m_k(x_l))"""
    L = len(widths)
    tr = hl.Keccak256Transcript.from_proof(proof)
    for v in [L, n, l] + widths:
        tr.common_field_element(v)
    for count in (sum(widths), L):
        mask = tr.read_field_element()
        tr.read_commitments(count - bin(mask).count("1"))
        tr.squeeze_challenge()  # beta, then gamma
    hl.verify_fractional_sum_check(n, [None] * L, [None] * L, tr)
    x_l = hl.verify_fractional_sum_check(l, [None] * L, [None] * L, tr)[4]
    tr.read_field_elements(sum(widths))
    return x_l, tr.read_field_elements(L)


@pytest.mark.parametrize("case,want", [("dup", None), ("one_row", [0, 0, 0, 16, 0, 0, 0, 0]), ("collide", None)])
def test_counts_through_the_proof(hl, ctx, kzg6, case, want):
    pp, vp = kzg6
    n, l, widths = lgr.CASES[case]
    tables = lgr.case_tables(case)
    rows = GOLDEN[case]["rows"][0]
    # the rule on the rows themselves: among equal table rows the LAST index takes every count
    last = {tuple(col[r] for col in tables[0]): r for r in range(1 << l)}
    m = [0] * (1 << l)
    for r in rows:
        m[last[tuple(col[r] for col in tables[0])]] += 1
    assert want is None or m == want
    if case == "dup":
        assert m[2] == m[5] == 0 and m[7] >= 5
    if case == "collide":
        assert m[1] >= 2 and m[6] >= 2
    lookups = _case(hl, ctx, case)
    proof = _prove(hl, pp, lookups)
    hl.logup_gkr_verify(vp, lookups, n, hl.Keccak256Transcript.from_proof(proof))
    x_l, m_e = _claims(hl, proof, n, l, widths)
    assert m_e == [evaluate(m, x_l)], "the committed multiplicities are not the counts of the last-index rule"


# ------------------------------------------------------------------ 5. refusals, and the ctx afterwards
def test_an_input_outside_the_table_is_invalid_snark_and_the_ctx_goes_on(hl, ctx, kzg6):
    pp, _ = kzg6
    for case, k in (("dup", 0), ("small_table", 1)):
        tables = lgr.case_tables(case)
        ins = lgr.inputs_of(tables, GOLDEN[case]["rows"])
        col = ins[k][0]
        col[-1] = next(v for v in range(1, 1000) if v not in tables[k][0])
        lookups = [hl.LogupLookup([hl.MultilinearPolynomial.new(ctx, c) for c in f], t) for f, t in zip(ins, tables)]
        t = hl.Keccak256Transcript()
        with pytest.raises(hl.InvalidSnark, match="Invalid lookup input"):
            hl.logup_gkr_prove(pp, lookups, t)
        assert _prove(hl, pp, _case(hl, ctx, case)).hex() == GOLDEN[case]["proof"]


def test_refusals_on_the_device_side(hl, ctx, kzg6):
    from halo2_lasso_amd import _ffi
    pp, _ = kzg6
    n, l, widths = 7, 3, [1]
    rng = random.Random(7)
    tables = [[[rng.randrange(P) for _ in range(1 << l)]]]
    lookups = _lookups(hl, ctx, tables, [[rng.randrange(1 << l) for _ in range(1 << n)]])
    with pytest.raises(hl.InvalidPcsParam):  # nv = 7 above the six variables of the SRS
        hl.logup_gkr_prove(pp, lookups, hl.Keccak256Transcript())
    good = _case(hl, ctx, "dup")
    arr, table_vars, keep = hl._logup_list(good, 4, True)
    t = hl.Keccak256Transcript()
    lib = ctx.lib
    assert lib.lh_logup_gkr_prove(ctx.h, None, arr, 1, 4, table_vars, t.p) == _ffi.LH_ERR_ARG  # NULL SRS
    assert lib.lh_logup_gkr_prove(ctx.h, pp.h, None, 1, 4, table_vars, t.p) == _ffi.LH_ERR_ARG  # NULL list
    assert lib.lh_logup_gkr_prove(ctx.h, pp.h, arr, 1, 4, table_vars, None) == _ffi.LH_ERR_ARG  # NULL transcript
    arr[0].d_inputs = None
    assert lib.lh_logup_gkr_prove(ctx.h, pp.h, arr, 1, 4, table_vars, t.p) == _ffi.LH_ERR_ARG  # NULL inputs
    assert b"d_inputs" in lib.lh_last_error() and not t.into_proof(), "refused before a byte is written"
    assert _prove(hl, pp, good).hex() == GOLDEN["dup"]["proof"]


# ------------------------------------------------------------------ 6. a size with many workgroups in every kernel
def test_larger_shape_verifies_under_both_switch_values(hl, ctx, kzg16):
    pp, vp = kzg16
    n, l, widths = LARGE
    rng = random.Random(1610)
    tables = [[[rng.randrange(P) for _ in range(1 << l)] for _ in range(w)] for w in widths]
    rows = [[rng.randrange(1 << l) for _ in range(1 << n)] for _ in widths]
    lookups = _lookups(hl, ctx, tables, rows)
    proofs = []
    for fused in (1, 0):
        with _option(hl, ctx, "logup_fused_leaves", fused):
            proofs.append(_prove(hl, pp, lookups))
    assert proofs[0] == proofs[1]
    t = hl.Keccak256Transcript.from_proof(proofs[0])
    hl.logup_gkr_verify(vp, lookups, n, t)
    assert t.remaining() == 0
