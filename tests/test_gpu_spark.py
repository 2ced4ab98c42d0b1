"""GPU: Spark (hl.spark_commit / hl.spark_open) - commitment and proof bytes against the golden file of the specification
(tests/spark_ref.py, tests/golden/spark.json), the host verifier, one handle opened many times, the route switches, the
launch records of its two kernels, refusals (the ctx goes on after each), and a size at which every kernel runs many
workgroups (n = 16: the value against the defining sum in big-integer arithmetic, the proofs against the host verifier)."""
import array
import ctypes as C
import json
import os
import random

import pytest

import logup_gkr_ref as lgr
import spark_ref as spr
from oracle.pyref.field import R_MOD as P

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "spark.json")))["cases"]
SS = [int(x, 16) for x in json.load(open(os.path.join(HERE, "golden", "lasso_tables.json")))["srs"]["ss"]]
SWITCHES = ["gkr_resident", "sc_tail", "sc_eq_factoring", "logup_fused_leaves"]
LARGE = (16, 10, 2)
ints = lambda xs: [int(x, 16) for x in xs]


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


_ENTRIES = {}


def _entries(case):
    """computed once per case and shared; callers copy before they damage a column"""
    if case not in _ENTRIES:
        _ENTRIES[case] = spr.case_entries(case)
    return _ENTRIES[case]


def _commit(hl, ctx, pp, dims, val, l):
    n = len(val).bit_length() - 1
    cols = [hl.U32Column(ctx.upload(array.array("I", d).tobytes()), n) for d in dims]
    return hl.spark_commit(ctx, pp, cols, hl.MultilinearPolynomial.new(ctx, val), l)


def _commit_case(hl, ctx, pp, case):
    return _commit(hl, ctx, pp, *_entries(case), spr.CASES[case][1])


def _points(case):
    return [ints(o["point"]) for o in GOLDEN[case]["openings"]]


def _same_as_golden(case, k, value, proof):
    o = GOLDEN[case]["openings"][k]
    return proof.hex() == o["proof"] and "%x" % value == o["value"]


def _one_var_still_proves(hl, ctx, pp):
    with _commit_case(hl, ctx, pp, "one_var") as poly:
        assert poly.commitment.hex() == GOLDEN["one_var"]["commitment"]
        return _same_as_golden("one_var", 0, *hl.spark_open(ctx, pp, poly, _points("one_var")[0]))


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
@pytest.mark.parametrize("case", list(spr.CASES))
def test_commitment_and_proof_bytes_equal_the_golden_and_verify(hl, ctx, kzg6, kzg16, case):
    pp, vp = kzg6 if case in spr.SMALL else kzg16
    n, l, c = spr.CASES[case]
    with _commit_case(hl, ctx, pp, case) as poly:
        assert poly.commitment.hex() == GOLDEN[case]["commitment"]
        assert (poly.num_vars, poly.dim_vars, poly.num_dims) == (n, l, c)
        for k, point in enumerate(_points(case)):
            value, proof = hl.spark_open(ctx, pp, poly, point)
            assert _same_as_golden(case, k, value, proof)
            hl.spark_verify(vp, n, l, c, poly.commitment, point, value, proof)
    mask = int.from_bytes(bytes.fromhex(GOLDEN[case]["commitment"])[:32], "big")
    if case == "distinct":  # both read_ts columns are zero and commit to the identity: polys 3 and 4
        assert mask == 0b11000
    if case == "zero_val":
        assert mask & 1 and value == 0


def test_one_handle_opens_many_times_in_either_order(hl, ctx, kzg6):
    pp, vp = kzg6
    case = "two_points"
    n, l, c = spr.CASES[case]
    pts = _points(case)
    poly = _commit_case(hl, ctx, pp, case)
    first = [hl.spark_open(ctx, pp, poly, pts[k]) for k in (0, 1)]
    again = [hl.spark_open(ctx, pp, poly, pts[k]) for k in (1, 0, 0)]
    assert first[0] == again[1] == again[2] and first[1] == again[0]
    assert _same_as_golden(case, 0, *first[0]) and _same_as_golden(case, 1, *first[1])
    # a second handle of the same entries, opened in the other order first: the same bytes
    other = _commit_case(hl, ctx, pp, case)
    assert other.commitment == poly.commitment
    assert hl.spark_open(ctx, pp, other, pts[1]) == first[1] and hl.spark_open(ctx, pp, other, pts[0]) == first[0]
    other.free()
    assert hl.spark_open(ctx, pp, poly, pts[1]) == first[1], "freeing one handle leaves the other alone"
    for k in (0, 1):
        hl.spark_verify(vp, n, l, c, poly.commitment, pts[k], *first[k])
    poly.free()
    poly.free()  # (twice is once)


# ------------------------------------------------------------------ 2. the route switches: same bytes
@pytest.mark.parametrize("case", ["matrix", "mid"])
def test_bytes_do_not_depend_on_the_switches(hl, ctx, kzg6, kzg16, case):
    pp, _ = kzg6 if case in spr.SMALL else kzg16
    point = _points(case)[0]
    with _commit_case(hl, ctx, pp, case) as poly:
        for name in SWITCHES:
            with _option(hl, ctx, name, 0):
                assert _same_as_golden(case, 0, *hl.spark_open(ctx, pp, poly, point)), name + " = 0"
        with _option(hl, ctx, "logup_fused_leaves", 1):
            assert _same_as_golden(case, 0, *hl.spark_open(ctx, pp, poly, point))
    with _option(hl, ctx, "logup_fused_leaves", 0):  # the commitment has no route to take
        with _commit_case(hl, ctx, pp, case) as poly:
            assert poly.commitment.hex() == GOLDEN[case]["commitment"]


# ------------------------------------------------------------------ 3. launch records
@pytest.mark.parametrize("case", ["matrix", "mid", "wide"])
def test_launch_records(hl, ctx, kzg6, kzg16, case):
    pp, _ = kzg6 if case in spr.SMALL else kzg16
    n, l, c = spr.CASES[case]
    N, M = 1 << n, 1 << l
    point = _points(case)[0]
    poly, recs = _profiled(hl, ctx, lambda: _commit_case(hl, ctx, pp, case))
    names = [r["name"] for r in recs]
    # the commit: the counters once for all dimensions, and two MSM batches - val, then the 3 c u32 columns over their own lengths
    assert names.count("lasso_counters") == 1 and not any(name.startswith("spark_") for name in names)
    digits = [r for r in recs if r["name"] == "msm_digits"]
    assert [(r["items"], r["muls"]) for r in digits] == [(max(N, M), max(N, M)), (c * (2 * N + M), 0)]
    for fused in (1, 0):
        with _option(hl, ctx, "logup_fused_leaves", fused):
            (value, proof), recs = _profiled(hl, ctx, lambda: hl.spark_open(ctx, pp, poly, point))
        assert _same_as_golden(case, 0, value, proof)
        by = {}
        for r in recs:
            by.setdefault(r["name"], []).append(r)
        # one launch each per opening: the memories with the value, the leaves of the 4 c trees
        assert [(r["items"], r["bytes"], r["muls"]) for r in by["spark_e"]] == [(N, (32 + 68 * c) * N, c * N)]
        up_n, up_l = bool(fused and n >= 12), bool(fused and l >= 12)
        ws_stored = not (up_n and n > l)
        assert [r["items"] for r in by["spark_leaves"]] == [c * (N + M)]
        assert by["spark_leaves"][0]["bytes"] == c * ((72 + 32 * up_n + 32 * ws_stored) * N + (100 + 32 * up_l) * M)
        assert by["spark_leaves"][0]["muls"] == c * ((1 + up_n) * N + (1 + up_l) * M)
        # a second (third ..) opening runs no counter, no sort of the index columns and no MSM over a committed column: every
        # point that goes through an MSM is a full-width scalar (E_j, the opening's quotients)
        assert "lasso_counters" not in by and not any(name.startswith(("memcheck_", "logup_")) for name in by)
        assert all(r["items"] == r["muls"] for r in by["msm_digits"])
        assert by["msm_digits"][0]["items"] == c * max(N, M), "the c memories, zero-padded to nv variables, in one batch"
    poly.free()


# ------------------------------------------------------------------ 4. refusals, and the ctx afterwards
def test_refusals_and_the_ctx_goes_on(hl, ctx, kzg6):
    from halo2_lasso_amd import _ffi
    pp, vp = kzg6
    lib = ctx.lib
    good = lambda: _one_var_still_proves(hl, ctx, pp)
    case = "matrix"
    n, l, c = spr.CASES[case]
    dims, val = _entries(case)
    for at, bad in ((0, 1 << l), (17, (1 << 31) | 3), ((1 << n) - 1, 0xFFFFFFFF)):  # an index = 2^l; bit 31 set; all ones
        for j in range(c):
            cols = [list(d) for d in dims]
            cols[j][at] = bad
            with pytest.raises(hl.ArgumentError, match="spark: index out of range"):
                _commit(hl, ctx, pp, cols, val, l)
            assert good()
    up = lambda cols: [hl.U32Column(ctx.upload(array.array("I", d).tobytes()), n) for d in cols]
    v = hl.MultilinearPolynomial.new(ctx, val)
    with pytest.raises(hl.ArgumentError, match="num_dims"):  # c = 4
        hl.spark_commit(ctx, pp, up(dims * 2), v, l)
    with pytest.raises(hl.ArgumentError, match="dim_vars"):  # l = 25
        hl.spark_commit(ctx, pp, up(dims), v, 25)
    assert good()
    with pytest.raises(hl.InvalidPcsParam):  # nv = 7 above the six variables of the SRS, by the dimensions
        hl.spark_commit(ctx, pp, up(dims), v, 7)
    assert good()
    rng = random.Random(7)
    big = [[rng.randrange(8) for _ in range(128)] for _ in range(2)]
    with pytest.raises(hl.InvalidPcsParam):  # ... and by the entries
        _commit(hl, ctx, pp, big, [rng.randrange(P) for _ in range(128)], 3)
    assert good()
    # through ctypes: the library's own answers on NULLs and shapes
    cols = up(dims)
    arr = C.cast(hl._ptr_array(cols), C.POINTER(C.POINTER(C.c_uint32)))
    holed = C.cast(hl._ptr_array([cols[0], 0]), C.POINTER(C.POINTER(C.c_uint32)))
    h = C.c_void_p()
    assert lib.lh_spark_commit(ctx.h, None, n, l, c, arr, v.ptr, C.byref(h)) == _ffi.LH_ERR_ARG  # NULL SRS
    assert lib.lh_spark_commit(ctx.h, pp.h, n, l, c, None, v.ptr, C.byref(h)) == _ffi.LH_ERR_ARG  # NULL list
    assert lib.lh_spark_commit(ctx.h, pp.h, n, l, c, holed, v.ptr, C.byref(h)) == _ffi.LH_ERR_ARG  # a NULL column
    assert b"d_dims[1]" in lib.lh_last_error()
    assert lib.lh_spark_commit(ctx.h, pp.h, n, l, c, arr, None, C.byref(h)) == _ffi.LH_ERR_ARG  # NULL val
    assert lib.lh_spark_commit(ctx.h, pp.h, n, l, c, arr, v.ptr, None) == _ffi.LH_ERR_ARG  # nowhere to put the handle
    assert lib.lh_spark_commit(ctx.h, pp.h, 0, l, c, arr, v.ptr, C.byref(h)) == _ffi.LH_ERR_ARG and not h.value
    assert good()
    assert lib.lh_spark_commit(ctx.h, pp.h, n, l, c, arr, v.ptr, C.byref(h)) == _ffi.LH_OK and h.value
    size = C.c_size_t(0)
    assert lib.lh_spark_commitment(h, None, C.byref(size)) == _ffi.LH_OK and size.value == 32 + 64 * (1 + 3 * c)
    out = (C.c_uint8 * size.value)()
    short = C.c_size_t(size.value - 1)
    assert lib.lh_spark_commitment(h, out, C.byref(short)) == _ffi.LH_ERR_ARG
    assert lib.lh_spark_commitment(h, out, C.byref(size)) == _ffi.LH_OK and bytes(out).hex() == GOLDEN[case]["commitment"]
    pt, val_out = hl._fr_array(_points(case)[0]), (hl.lh_fr * 1)()
    t = hl.Keccak256Transcript()
    assert lib.lh_spark_open(ctx.h, None, h, pt, val_out, t.p) == _ffi.LH_ERR_ARG
    assert lib.lh_spark_open(ctx.h, pp.h, None, pt, val_out, t.p) == _ffi.LH_ERR_ARG
    assert lib.lh_spark_open(ctx.h, pp.h, h, None, val_out, t.p) == _ffi.LH_ERR_ARG
    assert lib.lh_spark_open(ctx.h, pp.h, h, pt, None, t.p) == _ffi.LH_ERR_ARG
    assert lib.lh_spark_open(ctx.h, pp.h, h, pt, val_out, None) == _ffi.LH_ERR_ARG
    assert not t.into_proof(), "refused before a byte is written"
    t = hl.Keccak256Transcript()
    assert lib.lh_spark_open(ctx.h, pp.h, h, pt, val_out, t.p) == _ffi.LH_OK
    assert _same_as_golden(case, 0, hl._fr_list(val_out, 1)[0], t.into_proof())
    lib.lh_spark_free(ctx.h, h)
    # a freed handle is no longer one of the ctx's: refused without being read
    assert lib.lh_spark_open(ctx.h, pp.h, h, pt, val_out, hl.Keccak256Transcript().p) == _ffi.LH_ERR_ARG
    assert good()
    # open after free, and a point of the wrong length, in Python
    poly = _commit_case(hl, ctx, pp, case)
    with pytest.raises(hl.ArgumentError):
        hl.spark_open(ctx, pp, poly, _points(case)[0][:-1])
    poly.free()
    with pytest.raises(hl.ArgumentError, match="freed"):
        hl.spark_open(ctx, pp, poly, _points(case)[0])
    assert good()


# ------------------------------------------------------------------ 5. a size with many workgroups in every kernel
def test_larger_shape_round_trips(hl, ctx, kzg16):
    pp, vp = kzg16
    n, l, c = LARGE
    rng = random.Random(1610)
    dims = [[rng.randrange(1 << l) for _ in range(1 << n)] for _ in range(c)]
    val = [rng.randrange(P) for _ in range(1 << n)]
    points = [[rng.randrange(P) for _ in range(c * l)] for _ in range(2)]
    with _commit(hl, ctx, pp, dims, val, l) as poly:
        opened = []
        for fused in (1, 0):
            with _option(hl, ctx, "logup_fused_leaves", fused):
                opened.append([hl.spark_open(ctx, pp, poly, pt) for pt in points])
        assert opened[0] == opened[1]
        for pt, (value, proof) in zip(points, opened[0]):
            # 2^16 terms of big-integer arithmetic, independent of every kernel
            assert value == spr.sparse_eval(dims, val, l, pt)
            hl.spark_verify(vp, n, l, c, poly.commitment, pt, value, proof)
            with pytest.raises(hl.InvalidSnark, match="another value"):
                hl.spark_verify(vp, n, l, c, poly.commitment, pt, (value + 1) % P, proof)
        with pytest.raises(hl.InvalidSnark):  # the first proof is not about the second point
            hl.spark_verify(vp, n, l, c, poly.commitment, points[1], opened[0][1][0], opened[0][0][1])
