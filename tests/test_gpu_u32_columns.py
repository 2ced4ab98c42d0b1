"""The kernels that work on 32-bit columns without their field-element views (csrc/kernels_poly.hip) one call at a time
through the test-only entry lh_debug_u32_columns, against the big-integer references of tests/u32cols_ref.py.  Every
comparison is exact; the shapes are the smallest that reach each branch (listed in u32cols_ref.cases)."""
import ctypes as C
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import u32cols_ref as ur  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cus(ctx):
    n = ctx.compute_units()
    assert n >= 1
    return n


def sizes_of(op):
    """the operation's sizes in the order of its case list ("stride" where the size depends on the device)"""
    seen = []
    for kw in ur.cases(op, cus=256):
        s = "stride" if op in ("lincomb_bind2", "sc_round_u32_bind2") and ur.size_of(op, kw) == ur.stride_size(256) else ur.size_of(op, kw)
        if s not in seen:
            seen.append(s)
    return seen


def run_cases(ctx, op, cus, size):
    bad = ur.check_cases(ctx, op, cus, size)
    assert not bad, ur.report(bad)


@pytest.mark.parametrize("n", sizes_of("inner_products_small"))
def test_inner_products_small(ctx, cus, n):
    """every launch_ips<G> (count 1 .. 4), the partials buffer used again (5 = 4 + 1, 9 = 4 + 4 + 1), a wave and a
    workgroup and the 1024 x 256 grid cap from below, exactly and from above (2^18 + 1, 3 * 2^18 + 77: lanes stride)"""
    run_cases(ctx, "inner_products_small", cus, n)


def test_inner_products_small_accumulator_carries_into_limb_9(ctx):
    c, want = ur.closed_form_heavy(8 << 18)
    bad = ur.check(ctx, c, want)
    assert not bad, ur.report(bad)


@pytest.mark.parametrize("half", sizes_of("inner_products_small_half"))
def test_inner_products_small_half(ctx, cus, half):
    """the even / odd strided pseudo-columns against the eq table of y[1..]: <column, eq(y)> over all 2 half entries"""
    run_cases(ctx, "inner_products_small_half", cus, half)


@pytest.mark.parametrize("quads", sizes_of("inner_products_small_quads"))
def test_inner_products_small_quads(ctx, cus, quads):
    """even, odd, S2, S3 against the definition; with e0 = eq(y[1..]) also (1 - y0) even + y0 odd = <column, eq(y)>"""
    bad = []
    for kw in ur.cases("inner_products_small_quads", cus, quads):
        c = ur.build("inner_products_small_quads", **kw)
        want = ur.reference(c)
        bad += ur.check(ctx, c, want)
        if c.y is not None and not bad:
            bad += ur.quads_identity(c, want["sums"])  # (the device's sums equal these)
    assert not bad, ur.report(bad)


@pytest.mark.parametrize("quads", sizes_of("inner_products_quads"))
def test_inner_products_quads(ctx, cus, quads):
    """launch groups of two columns: both short (the launch covers most < quads), short with full, a lone tail; lengths 0,
    4, 4 (quads - 1), 4 quads and 8 quads (clamped to the table)"""
    run_cases(ctx, "inner_products_quads", cus, quads)


@pytest.mark.parametrize("n", sizes_of("lincomb_mixed"))
def test_lincomb_mixed(ctx, cus, n):
    run_cases(ctx, "lincomb_mixed", cus, n)


@pytest.mark.parametrize("half", sizes_of("lincomb_fold_small"))
def test_lincomb_fold_small(ctx, cus, half):
    run_cases(ctx, "lincomb_fold_small", cus, half)


@pytest.mark.parametrize("count", [0, ur.LCF_MAX + 1])
def test_lincomb_fold_small_not_taken(ctx, count):
    """no columns, or more than a launch takes: reported as not taken (the caller's cue for the other route), not an error"""
    c = ur.build("lincomb_fold_small", half=64, count=count)
    assert not ur.reference(c)["taken"]
    bad = ur.check(ctx, c)
    assert not bad, ur.report(bad)


@pytest.mark.parametrize("size", sizes_of("lincomb_bind2"))
def test_lincomb_bind2(ctx, cus, size):
    """2 size <= 256: the single-workgroup publish; 129: the first two-workgroup finish; the last size strides the capped
    grid.  The bound table, q(0) and q(1) are all compared"""
    run_cases(ctx, "lincomb_bind2", cus, size)


@pytest.mark.parametrize("size", sizes_of("sc_round_u32_bind2"))
def test_sc_round_u32_bind2(ctx, cus, size):
    run_cases(ctx, "sc_round_u32_bind2", cus, size)


def back_to_back_cases(cus):
    """a few cases of every operation: grids of one workgroup, of two and capped ones, with and without a finish"""
    picks = [("lincomb_bind2", dict(size=64, count=2, rot=1)), ("inner_products_small", dict(n=257, count=5, rot=0)),
             ("lincomb_bind2", dict(size=ur.stride_size(cus), count=1, rot=0)), ("lincomb_mixed", dict(n=257, num_fr=1, num_sm=2, rot=1)),
             ("sc_round_u32_bind2", dict(size=129, pattern="uniform", rot=0)), ("inner_products_quads", dict(quads=257, lens=("short", "full", "long"), rot=0)),
             ("lincomb_bind2", dict(size=129, count=3, rot=2)), ("lincomb_fold_small", dict(half=257, count=2, x="random", rot=2)),
             ("sc_round_u32_bind2", dict(size=ur.stride_size(cus), pattern="ones", rot=0)), ("inner_products_small_quads", dict(quads=257, pattern="uniform")),
             ("sc_round_u32_bind2", dict(size=64, pattern="sparse", rot=4)), ("inner_products_small_half", dict(half=257, count=3, rot=0))]
    return [ur.build(op, **kw) for op, kw in picks]


def test_back_to_back_calls_on_one_ctx(ctx, cus):
    """48 calls in a row on one ctx, operations, grid sizes and finish kinds alternating, every result checked: the ticket
    base, the lane tags, the pinned staging block and the partials buffers carry over from call to call"""
    staged = [ur.Staged(ctx, c) for c in back_to_back_cases(cus)]
    want = [ur.reference(s.c) for s in staged]
    bad = []
    try:
        for turn in range(4):
            order = range(len(staged)) if turn % 2 == 0 else [(5 * i + turn) % len(staged) for i in range(len(staged))]
            for i in order:
                st = staged[i].launch()
                if st != ur.LH_OK:
                    bad.append("call of turn %d, %s: status %d: %s" % (turn, staged[i].c.what(), st, ctx.lib.lh_last_error().decode()))
                    continue
                lines, got = staged[i].results()
                bad += ["turn %d: %s" % (turn, ln) for ln in lines + ur.compare(staged[i].c, got, want[i])]
    finally:
        for s in staged:
            s.free()
    assert not bad, ur.report(bad)


def test_bind2_and_back_to_back_under_the_ticket_finish():
    """LH_FIN_LANES_MIN_BYTES is read once per process: the two bind2 kernels and the back-to-back calls again in a child
    process in which no launch hands its sums over in lanes (the ticket finish; by default every launch of more than one
    workgroup uses the lanes)"""
    res = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_u32_columns.py", "-m", "gpu", "-x", "-q", "-k",
                          "test_lincomb_bind2 or test_sc_round_u32_bind2 or test_back_to_back"], cwd=ROOT,
                         env=dict(os.environ, LH_FIN_LANES_MIN_BYTES="-1"), capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]


def test_refused_arguments_leave_the_ctx_working(ctx):
    """a misaligned column, a length that is no multiple of 4 and a count above the cap are LH_ERR_ARG before anything is
    launched; the ctx computes afterwards"""
    from halo2_lasso_amd import _ffi
    lib = ctx.lib

    def status(c, edit):
        s = ur.Staged(ctx, c)
        try:
            edit(s)
            st = s.launch()
            bad, got = s.results()
            return st, bad, got["untouched"]
        finally:
            s.free()

    def misalign(s):
        s.keep[0][0] = s.cols.ptr(0) + 4

    def odd_length(s):
        s.keep[1][0] = s.c.lens[0] - 2

    refused = {}
    for op, kw in (("inner_products_small_quads", dict(quads=64, pattern="uniform")), ("sc_round_u32_bind2", dict(size=64, pattern="uniform")),
                   ("inner_products_quads", dict(quads=64, lens=("full", "full"))), ("lincomb_bind2", dict(size=64, count=2))):
        refused[op + ", misaligned"] = status(ur.build(op, **kw), misalign)
        if op in ("inner_products_quads", "lincomb_bind2"):
            refused[op + ", length 4 q - 2"] = status(ur.build(op, **kw), odd_length)
    refused["lincomb_bind2, 25 columns"] = status(ur.build("lincomb_bind2", size=2, count=ur.LCB_MAX + 1), lambda s: None)
    refused["lincomb_bind2, no columns"] = status(ur.build("lincomb_bind2", size=2, count=0), lambda s: None)
    refused["lincomb_mixed, 25 columns"] = status(ur.build("lincomb_mixed", n=4, num_fr=0, num_sm=ur.LCM_MAX_SMALL + 1), lambda s: None)
    refused["lincomb_mixed, 9 tables"] = status(ur.build("lincomb_mixed", n=4, num_fr=ur.LCM_MAX_FR + 1, num_sm=1), lambda s: None)
    for what, (st, bad, untouched) in refused.items():
        assert st == ur.LH_ERR_ARG and not bad and untouched, (what, st, bad, untouched, lib.lh_last_error())
    # an unknown operation, n = 0, null argument blocks
    c = ur.build("inner_products_small", n=4, count=1)
    s = ur.Staged(ctx, c)
    try:
        assert lib.lh_debug_u32_columns(ctx.h, len(ur.OPS), C.byref(s.args)) == ur.LH_ERR_ARG
        assert lib.lh_debug_u32_columns(ctx.h, -1, C.byref(s.args)) == ur.LH_ERR_ARG
        assert lib.lh_debug_u32_columns(ctx.h, 0, None) == ur.LH_ERR_ARG
        s.args.n = 0
        assert s.launch() == ur.LH_ERR_ARG
        s.args.n, s.args.out_host = 4, C.cast(None, C.POINTER(_ffi.lh_fr))
        assert s.launch() == ur.LH_ERR_ARG and b"null argument" in lib.lh_last_error()
    finally:
        s.free()
    # ... and the ctx still computes, finish included
    bad = ur.check(ctx, ur.build("lincomb_bind2", size=129, count=2)) + ur.check(ctx, c)
    assert not bad, ur.report(bad)
