"""The kernel that makes the quad sums of all the columns of a point in one launch (csrc/kernels_poly.hip k_quad_sums), alone,
through the test-only entry lh_debug_u32_columns (operation QUAD_SUMS), against the big-integer reference of
tests/u32cols_ref.py:  d_out[4 k + t] = sum_{q < quads} (e0[2q] + e0[2q+1]) col_k[4 q + t],  entries from lens[k] on zero.

Every comparison is exact.  The device memory is u32cols_ref's: guard words around every region, the output pre-filled with
the guard pattern, the inputs read back unchanged, non-zero filler behind a column that is shorter than the table.

Shapes: 1 quad (one lane), 255 (one lane short of the workgroup's 256-lane stride), 1027 (4 x 256 + 3: three lanes hold one
quad more than the others, the last wave's lanes hold fewer), 2^12 (more than one workgroup: several rows of partials per
sum); 1, 2, 3 and 12 columns, and 25 (more than one launch takes: 24 + 1)."""
import ctypes as C
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import u32cols_ref as ur  # noqa: E402

pytestmark = pytest.mark.gpu

LENS = ("full", "short", "zero", "long", "four")  # names of ur.quad_lens()


def op_code():
    from halo2_lasso_amd import _ffi
    return _ffi.LH_U32_OPS.index("quad_sums")


def e0_table(quads, seed):
    """2 quads eq entries: random ones with the three stored edges (ur.fr_random), and - where there is room - the canonical
    values 0 and r - 1, alone and as a pair whose sum wraps around r"""
    e0 = ur.fr_random(2 * quads, ("e0", quads, seed)).ints()
    if quads >= 4:
        e0[2], e0[3] = 0, ur.R_MOD - 1          # E_1[1] = r - 1
        e0[4], e0[5] = ur.R_MOD - 1, ur.R_MOD - 1  # E_1[2] = r - 2 after one wrap
        e0[6], e0[7] = 0, 0                     # E_1[3] = 0
    return ur.FrTable.from_ints(e0)


def build(quads, lens, rot):
    """a case staged like inner_products_quads (4 sums per column in d_out), with d_weights = e0 of 2 quads entries"""
    ln = [ur.quad_lens(quads)[name] for name in lens]
    cols = [ur.column(ur._pick(ur.PATTERNS, k + rot), ln[k], max(ln[k], 4 * quads), ("qs", quads, tuple(lens), k)) for k in range(len(ln))]
    return ur.Case("inner_products_quads", "quad_sums: quads=%d, lens %s, patterns from %s" % (
        quads, "/".join(lens) if len(lens) <= 6 else "%d columns" % len(lens), ur._pick(ur.PATTERNS, rot)), quads, cols, ln,
        e0_table(quads, len(lens)))


def reference(c):
    e0 = c.weights.ints()
    e1 = ur.FrTable.from_ints([(e0[2 * q] + e0[2 * q + 1]) % ur.R_MOD for q in range(c.n)])
    return {"sums": None, "taken": True,
            "table": [ur.dot(e1, col[:min(ln, 4 * c.n)][t::4]) for col, ln in zip(c.cols, c.lens) for t in range(4)]}


def check(ctx, c):
    s = ur.Staged(ctx, c)
    try:
        st = ctx.lib.lh_debug_u32_columns(ctx.h, op_code(), C.byref(s.args))
        if st != ur.LH_OK:
            return ["%s: lh_debug_u32_columns returned %d: %s" % (c.what(), st, ctx.lib.lh_last_error().decode())]
        bad, got = s.results()
        return bad + ur.compare(c, got, reference(c))
    finally:
        s.free()


def arrangements():
    """1 column: every length alone; 2, 3, 12: the lengths in turn from a different start each - every count has a column
    shorter than the table and (from 2 on) one of length 0 beside full ones"""
    out = [(name,) for name in LENS]
    for count, start in ((2, 1), (2, 0), (3, 0), (3, 2), (12, 0), (12, 3)):
        out.append(tuple(ur._pick(LENS, start + k) for k in range(count)))
    return out


@pytest.mark.parametrize("quads", [1, 255, 1027, 1 << 12])
def test_quad_sums(ctx, quads):
    bad = []
    for j, lens in enumerate(arrangements()):
        bad += check(ctx, build(quads, lens, j))
    assert not bad, ur.report(bad)


def test_quad_sums_more_columns_than_a_launch_takes(ctx):
    """25 columns: a launch of 24 and one of 1 share the partials buffer"""
    lens = tuple(ur._pick(LENS, k) for k in range(25))
    bad = check(ctx, build(255, lens, 1))
    assert not bad, ur.report(bad)


def test_quad_sums_refused_arguments(ctx):
    """a misaligned column, a length that is no multiple of 4, a null length list: LH_ERR_ARG before anything is launched, d_out
    untouched; 8 - the gap in front of this operation's code - is no operation"""
    c = build(64, ("full", "full"), 0)

    def status(edit, op=None):
        s = ur.Staged(ctx, c)
        try:
            edit(s)
            st = ctx.lib.lh_debug_u32_columns(ctx.h, op_code() if op is None else op, C.byref(s.args))
            bad, got = s.results()
            return st, bad, got["untouched"]
        finally:
            s.free()

    def misalign(s):
        s.keep[0][0] = s.cols.ptr(0) + 4

    def odd_length(s):
        s.keep[1][1] = c.lens[1] - 2

    def no_lens(s):
        s.args.lens = C.cast(None, C.POINTER(C.c_size_t))

    for what, got in (("misaligned", status(misalign)), ("length 4 q - 2", status(odd_length)), ("no lens", status(no_lens)),
                      ("operation 8", status(lambda s: None, op=8))):
        assert got[0] == ur.LH_ERR_ARG and not got[1] and got[2], (what, got, ctx.lib.lh_last_error())
    bad = check(ctx, c)  # ... and the ctx still computes
    assert not bad, ur.report(bad)
