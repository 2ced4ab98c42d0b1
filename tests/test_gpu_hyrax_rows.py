"""GPU: the row kernels of a Hyrax commit (csrc/kernels_hyrax.hip) on their own, through lh_g1_rows_msm and, for a batch of
columns in one call, through lh_hyrax_batch_commit.  Everything is exact: the expected points come from
oracle.pyref.curve.msm where a case has at most 64 terms in all, elsewhere from the library's variable_base_msm /
variable_base_msm_u32 row by row (the bucket MSM of csrc/msm.hip: independent code, tested against the oracles).

Sizes and the boundaries they sit on:
  windows        8-bit digits (cbits = 8), signed for Fr: 32 windows, buckets 1..128, digit 128 stays positive and 129 carries;
                 unsigned for u32: ceil(bits / 8) windows, buckets 1..255, two buckets per thread
  segment        one workgroup takes S = 256 columns of an Fr row and S = 2048 columns of a u32 row: row_len S / 2, S, 2 S, 4 S
                 are rows of half a segment and of one, two and four segments (the second and fourth go through the kernel
                 that adds the segments' points up)
  workgroup      128 threads: row_len 1, 2, 8, 64 leave most of them without a column, 256 gives each two
  launch         48 columns per launch: a batch of 50 tables is two launches
  rows           1, 2, 3 and 300 rows (300 workgroups; the normalisation inverts 8 points at a time: a partial last batch)
  beyond n       rows that lie wholly beyond a column's entries (a short column inside a taller table: no workgroup, (0, 0))
                 cannot be expressed through lh_g1_rows_msm, whose rows are ceil(n / row_len): they are covered through the
                 Lasso prover in tests/test_gpu_hyrax_provers.py (the `and` input and the at-size run)
  n              rows * row_len, one less (the last entry of the last row absent) and row_len - 1 less (the last row is one entry)
"""
import random

import pytest

from oracle.pyref import curve
from oracle.pyref.field import R_MOD as P

pytestmark = pytest.mark.gpu

CBITS = 8
S_FR, S_U32 = 256, 2048


@pytest.fixture(scope="module")
def gens(hl, ctx):
    """8192 generators of a real param, as points and on the device"""
    g, _ = hl.Ipa.setup(ctx, 8192).download()
    return g, ctx.upload(b"".join(hl.g1_to_bytes(p) for p in g))


def _upload_points(hl, ctx, pts):
    return ctx.upload(b"".join(hl.g1_to_bytes(p) for p in pts))


def _expected(hl, ctx, scalars, sbuf, n, row_len, bases, bbuf, u32):
    """the rows' sums: the Python curve where the case is small, the library's bucket MSM row by row elsewhere"""
    rows = (n + row_len - 1) // row_len
    if n <= 64:
        return [curve.msm(scalars[r * row_len:min(n, (r + 1) * row_len)], bases[:min(n, (r + 1) * row_len) - r * row_len])
                for r in range(rows)]
    width = 4 if u32 else 32
    out = []
    for r in range(rows):
        cnt = min(n, (r + 1) * row_len) - r * row_len
        view = hl.DeviceBuffer(ctx, cnt * width, ptr=sbuf.ptr + r * row_len * width)
        out.append(hl.variable_base_msm_u32(ctx, view, bbuf, cnt) if u32 else hl.variable_base_msm(ctx, view, bbuf, cnt))
    return out


def _planted_fr():
    """digit edges of the first, a middle and the top window: all-ones below the window (a carry chain into it), the window's
    lowest bit, and the half 2^(8 j - 1) = digit 128 of the window below (the largest positive digit); 2^248 - 1 carries
    through every window into the last one"""
    vals = [0, 1, P - 1, 127, 128, 129, 255, 256]
    for j in (1, 16, 31):
        vals += [(1 << (CBITS * j)) - 1, 1 << (CBITS * j), 1 << (CBITS * j - 1), (1 << (CBITS * j - 1)) + 1]
    return vals


def _fr_scalars(rng, n):
    s = [rng.randrange(P) for _ in range(n)]
    planted = _planted_fr()
    for i, pos in enumerate(rng.sample(range(n), min(n, len(planted)))):
        s[pos] = planted[i]
    return s


def _run_fr(hl, ctx, scalars, n, row_len, bases, bbuf):
    sbuf = ctx.upload(hl.frs_to_bytes(scalars[:n]))
    got = hl.Hyrax.rows_msm(ctx, sbuf, n, row_len, bbuf)
    assert got == _expected(hl, ctx, scalars, sbuf, n, row_len, bases, bbuf, False)
    return got


def _ns(rows, row_len):
    return sorted({rows * row_len, rows * row_len - 1, rows * row_len - (row_len - 1)} - {0})


@pytest.mark.parametrize("row_len,rows", [(1, 1), (1, 3), (2, 1), (2, 2), (2, 300), (8, 3), (64, 2), (S_FR // 2, 3), (S_FR, 2),
                                          (2 * S_FR, 3), (4 * S_FR, 2)])
def test_fr_rows_of_every_shape(hl, ctx, gens, row_len, rows):
    g, gbuf = gens
    rng = random.Random(9000 + 31 * row_len + rows)
    scalars = _fr_scalars(rng, rows * row_len)
    for n in _ns(rows, row_len):
        got = _run_fr(hl, ctx, scalars, n, row_len, g, gbuf)
        assert len(got) == (n + row_len - 1) // row_len


def test_fr_every_planted_scalar_alone_in_a_row(hl, ctx, gens):
    """row_len 1: each row is one scalar times g[0], against the Python curve"""
    g, gbuf = gens
    scalars = _planted_fr()
    sbuf = ctx.upload(hl.frs_to_bytes(scalars))
    got = hl.Hyrax.rows_msm(ctx, sbuf, len(scalars), 1, gbuf)
    fb = curve.FixedBase(g[0])
    assert got == [fb.mul(s) if s else None for s in scalars]
    assert got[0] is None


def test_fr_planted_rows_in_one_call(hl, ctx, gens):
    """a row of equal scalars (one bucket per window takes every term), an all-zero row between ordinary ones (the identity,
    (0, 0)), a row with one nonzero entry, a row of r - 1"""
    g, gbuf = gens
    row_len = 64
    rng = random.Random(9101)
    eq = rng.randrange(P)
    rows = [[eq] * row_len, [rng.randrange(P) for _ in range(row_len)], [0] * row_len, [rng.randrange(P) for _ in range(row_len)],
            [0] * 17 + [rng.randrange(1, P)] + [0] * (row_len - 18), [P - 1] * row_len]
    got = _run_fr(hl, ctx, [s for r in rows for s in r], len(rows) * row_len, row_len, g, gbuf)
    assert got[2] is None and all(got[i] is not None for i in (0, 1, 3, 4, 5))
    assert got[4] == curve.mul(g[17], rows[4][17])
    assert got[5] == curve.neg(curve.msm([1] * row_len, g[:row_len]))


@pytest.mark.parametrize("row_len", [8, 64, 2 * S_FR])
def test_fr_all_bases_the_same_point(hl, ctx, row_len):
    """accumulating a bucket hits P + P at once, and the reduction adds equal points"""
    rng = random.Random(9200 + row_len)
    pt = curve.mul(curve.G1_GEN, rng.randrange(1, P))
    bbuf = _upload_points(hl, ctx, [pt] * row_len)
    eq = rng.randrange(P)
    rows = [[rng.randrange(P) for _ in range(row_len)], [eq] * row_len, [1] * row_len, [(P - 1) // 2, (P + 1) // 2] * (row_len // 2)]
    sbuf = ctx.upload(hl.frs_to_bytes([s for r in rows for s in r]))
    got = hl.Hyrax.rows_msm(ctx, sbuf, len(rows) * row_len, row_len, bbuf)
    assert got == [curve.mul(pt, sum(r) % P) if sum(r) % P else None for r in rows]
    assert got[3] is None


@pytest.mark.parametrize("row_len", [8, 64])
def test_fr_opposite_bases_with_equal_scalars(hl, ctx, row_len):
    """pairs (P, -P) with equal scalars: every bucket passes through the identity; one unpaired term in the second row"""
    rng = random.Random(9300 + row_len)
    fb = curve.FixedBase(curve.G1_GEN)
    half = [fb.mul(rng.randrange(1, P)) for _ in range(row_len // 2)]
    bases = [q for p in half for q in (p, curve.neg(p))]
    bbuf = _upload_points(hl, ctx, bases)
    pair = [rng.randrange(1, P) for _ in range(row_len // 2)]
    row0 = [s for v in pair for s in (v, v)]
    row1 = list(row0)
    row1[5] = (row1[5] + 3) % P  # the partner of entry 4: the row's sum is 3 * bases[5]
    same = rng.randrange(1, P)
    sbuf = ctx.upload(hl.frs_to_bytes(row0 + row1 + [same] * row_len))
    got = hl.Hyrax.rows_msm(ctx, sbuf, 3 * row_len, row_len, bbuf)
    assert got == [None, curve.mul(bases[5], 3), None]


def _run_u32(hl, ctx, vals, n, row_len, bits, bases, bbuf):
    import numpy as np
    sbuf = ctx.upload(np.asarray(vals[:n], dtype=np.uint32).tobytes())
    got = hl.Hyrax.rows_msm(ctx, sbuf, n, row_len, bbuf, u32=True, bits=bits)
    assert got == _expected(hl, ctx, vals, sbuf, n, row_len, bases, bbuf, True)
    return got


@pytest.mark.parametrize("bits", [1, 8, 9, 16, 17, 32])
def test_u32_columns_of_every_width(hl, ctx, gens, bits):
    """values up to 2^bits - 1 (planted, with 0 and the byte edges below it), rows of 64 with a partial last row"""
    g, gbuf = gens
    rng = random.Random(9400 + bits)
    row_len, rows = 64, 3
    top = (1 << bits) - 1
    vals = [rng.randrange(top + 1) for _ in range(rows * row_len)]
    for i, v in enumerate([top, 0, top, 1, 255 & top, 256 & top, 65535 & top, 65536 & top, top >> 1]):
        vals[7 * i + 3] = v
    for n in _ns(rows, row_len):
        _run_u32(hl, ctx, vals, n, row_len, bits, g, gbuf)
    _run_u32(hl, ctx, [top] * (rows * row_len), rows * row_len - 5, row_len, bits, g, gbuf)  # an all-equal column


@pytest.mark.parametrize("row_len,rows", [(1, 3), (2, 300), (8, 2), (S_U32 // 2, 3), (S_U32, 2), (2 * S_U32, 2), (4 * S_U32, 1)])
def test_u32_rows_of_every_shape(hl, ctx, gens, row_len, rows):
    g, gbuf = gens
    rng = random.Random(9500 + 31 * row_len + rows)
    vals = [rng.randrange(1 << 16) for _ in range(rows * row_len)]
    for n in _ns(rows, row_len):
        _run_u32(hl, ctx, vals, n, row_len, 16, g, gbuf)


def test_u32_zero_rows_and_repeated_small_values(hl, ctx, gens):
    """a Lasso counter column: a few small values repeated, a row of zeros in the middle: (0, 0)"""
    g, gbuf = gens
    rng = random.Random(9600)
    row_len = 256
    vals = [rng.choice([0, 1, 2, 3]) for _ in range(row_len)] + [0] * row_len + [rng.choice([0, 5]) for _ in range(row_len)]
    got = _run_u32(hl, ctx, vals, 3 * row_len, row_len, 3, g, gbuf)
    assert got[1] is None and got[0] is not None and got[2] is not None


def test_a_batch_of_three_columns_in_one_call(hl, ctx):
    """lh_hyrax_batch_commit hands all rows of all polys to ONE call of the row kernels: three tables of 2^8 entries (16 rows of
    16), an all-zero row and an all-zero table among them, on both commit routes"""
    rng = random.Random(9700)
    n = 8
    params = hl.Hyrax.setup(ctx, 1 << n, 1)
    pp = hl.Hyrax.trim(params, 1 << n, 1)
    g, _ = params.download()
    gbuf = _upload_points(hl, ctx, g)
    row_len = 1 << pp.row_num_vars
    tables = [[rng.randrange(P) for _ in range(1 << n)] for _ in range(2)] + [[0] * (1 << n)]
    tables[1][3 * row_len:4 * row_len] = [0] * row_len
    polys = [hl.MultilinearPolynomial.new(ctx, t) for t in tables]
    want = []
    for t in tables:
        sbuf = ctx.upload(hl.frs_to_bytes(t))
        want.append(_expected(hl, ctx, t, sbuf, 1 << n, row_len, g, gbuf, False))
    assert want[1][3] is None and want[2] == [None] * pp.num_chunks
    try:
        for route in (1, 0):
            hl.set_option(ctx, "hyrax_rows", route)
            assert hl.Hyrax.batch_commit(pp, polys) == want
    finally:
        hl.set_option(ctx, "hyrax_rows", 1)


def test_a_batch_of_more_columns_than_one_launch_takes(hl, ctx):
    """the descriptors of 48 columns travel with one launch: 50 tables of 2^4 entries (4 rows of 4) are two launches, against
    the 200 jobs of the msm_batch route"""
    rng = random.Random(9750)
    n = 4
    pp = hl.Hyrax.trim(hl.Hyrax.setup(ctx, 1 << n, 1), 1 << n, 1)
    tables = [[rng.randrange(P) for _ in range(1 << n)] for _ in range(50)]
    tables[49][4:8] = [0] * 4
    polys = [hl.MultilinearPolynomial.new(ctx, t) for t in tables]
    try:
        hl.set_option(ctx, "hyrax_rows", 0)
        old = hl.Hyrax.batch_commit(pp, polys)
        hl.set_option(ctx, "hyrax_rows", 1)
        new = hl.Hyrax.batch_commit(pp, polys)
    finally:
        hl.set_option(ctx, "hyrax_rows", 1)
    assert new == old and len(new) == 50 and new[49][1] is None and None not in new[48]


@pytest.mark.parametrize("n,batch_size", [(14, 1), (16, 1)])
def test_both_commit_routes_agree(hl, ctx, n, batch_size):
    """128 rows of 128 and 256 rows of 256: the row kernels against one msm_batch job per row"""
    pp = hl.Hyrax.trim(hl.Hyrax.setup(ctx, 1 << n, batch_size), 1 << n, batch_size)
    rng = random.Random(9800 + n)
    polys = [hl.MultilinearPolynomial.new(ctx, [rng.randrange(P) for _ in range(1 << n)]) for _ in range(2)]
    try:
        hl.set_option(ctx, "hyrax_rows", 0)
        old = hl.Hyrax.batch_commit(pp, polys)
        hl.set_option(ctx, "hyrax_rows", 1)
        new = hl.Hyrax.batch_commit(pp, polys)
    finally:
        hl.set_option(ctx, "hyrax_rows", 1)
    assert new == old and len(new) == 2 and len(new[0]) == pp.num_chunks and None not in new[0]


def test_rows_msm_arguments(hl, ctx, gens):
    _, gbuf = gens
    sbuf = ctx.upload(bytes(64))
    lib, h = ctx.lib, ctx.h
    out = (hl._ffi.lh_g1 * 2)()
    bad = [lib.lh_g1_rows_msm(None, sbuf.ptr, 0, 0, 2, 2, gbuf.ptr, out), lib.lh_g1_rows_msm(h, None, 0, 0, 2, 2, gbuf.ptr, out),
           lib.lh_g1_rows_msm(h, sbuf.ptr, 0, 0, 2, 2, None, out), lib.lh_g1_rows_msm(h, sbuf.ptr, 0, 0, 2, 2, gbuf.ptr, None),
           lib.lh_g1_rows_msm(h, sbuf.ptr, 0, 0, 2, 0, gbuf.ptr, out), lib.lh_g1_rows_msm(h, sbuf.ptr, 1, 0, 2, 2, gbuf.ptr, out),
           lib.lh_g1_rows_msm(h, sbuf.ptr, 1, 33, 2, 2, gbuf.ptr, out)]
    assert bad == [hl._ffi.LH_ERR_ARG] * len(bad)
    assert lib.lh_g1_rows_msm(h, None, 0, 0, 0, 2, None, None) == hl._ffi.LH_OK  # nothing to do
    assert hl.Hyrax.rows_msm(ctx, sbuf, 2, 2, gbuf) == [None]
