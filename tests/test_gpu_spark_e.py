"""GPU: the memory kernel of a Spark opening on its own (lh_debug_spark_e; csrc/kernels_spark.hip spark_e) against a
big-integer restatement: E_j[k] = eq(r_j, dim_j[k]) - a 32-byte gather by a u32 index from the eq table of the point's
j-th part - and v = sum_k val[k] prod_j E_j[k].  Both are compared exactly: field elements, no tolerance.

Shapes (n, l, c): (1, 1, 1) two entries in one workgroup; (10, 1, 2) a two-entry table hit by every lane; (10, 10, 2) four
workgroups; (11, 16, 1) a 2 MiB table - next to the columns it no longer sits in one L2; (13, 9, 3) three dimensions, 32
workgroups, so the final sum adds many partial sums."""
import array
import random

import pytest

from oracle.pyref.field import R_MOD as P

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (10, 1, 2), (10, 10, 2), (11, 16, 1), (13, 9, 3)]


def eq_table(r):
    """eq(r, m) for every m < 2^len(r), coordinate i belongs to bit i of m: doubling, one coordinate at a time"""
    table = [1]
    for x in r:
        table = [t * (1 - x) % P for t in table] + [t * x % P for t in table]
    return table


def restate(dims, val, l, point):
    T = [eq_table(point[j * l:(j + 1) * l]) for j in range(len(dims))]
    E = [[T[j][d] for d in col] for j, col in enumerate(dims)]
    v = 0
    for k in range(len(val)):
        t = val[k]
        for e in E:
            t = t * e[k] % P
        v = (v + t) % P
    return E, v


def test_the_restatement_is_the_eq_polynomial():
    r = [3, 5, 7]
    for m in range(8):
        want = 1
        for i, x in enumerate(r):
            want = want * (x if (m >> i) & 1 else 1 - x) % P
        assert eq_table(r)[m] == want


_DATA = {}


def _data(shape):
    """computed once per shape and shared"""
    if shape not in _DATA:
        n, l, c = shape
        rng = random.Random(repr(("spark_e", shape)))
        dims = [[rng.randrange(1 << l) for _ in range(1 << n)] for _ in range(c)]
        val = [rng.randrange(P) for _ in range(1 << n)]
        point = [rng.randrange(P) for _ in range(c * l)]
        _DATA[shape] = (dims, val, point) + restate(dims, val, l, point)
    return _DATA[shape]


def _run(hl, ctx, dims, val, l, point, offset=0):
    """offset: every index column starts that many words into its buffer"""
    n = len(val).bit_length() - 1
    bufs = [ctx.upload(array.array("I", [0] * offset + list(d)).tobytes()) for d in dims]
    cols = [hl.DeviceBuffer(ctx, 4 << n, ptr=b.ptr + 4 * offset) for b in bufs]
    return hl.spark_e(ctx, cols, hl.MultilinearPolynomial.new(ctx, val), l, point)


@pytest.mark.parametrize("shape", SHAPES)
def test_memories_and_value_are_exact(hl, ctx, shape):
    dims, val, point, E, v = _data(shape)
    got_E, got_v = _run(hl, ctx, dims, val, shape[1], point)
    assert got_v == v
    assert got_E == E


@pytest.mark.parametrize("shape", [(10, 10, 2), (13, 9, 3)])
def test_all_indices_equal(hl, ctx, shape):
    n, l, c = shape
    _, val, point, _, _ = _data(shape)
    dims = [[(1 << l) - 1 - j] * (1 << n) for j in range(c)]  # one cell per dimension, the last ones of the table
    E, v = restate(dims, val, l, point)
    got_E, got_v = _run(hl, ctx, dims, val, l, point)
    assert got_v == v and got_E == E
    assert all(len(set(e)) == 1 for e in got_E)


@pytest.mark.parametrize("shape", [(1, 1, 1), (10, 10, 2)])
def test_unaligned_index_columns(hl, ctx, shape):
    dims, val, point, E, v = _data(shape)
    got_E, got_v = _run(hl, ctx, dims, val, shape[1], point, offset=1)
    assert got_v == v and got_E == E


def test_an_index_out_of_range_is_refused_and_the_ctx_goes_on(hl, ctx):
    shape = (10, 10, 2)
    dims, val, point, E, v = _data(shape)
    for bad in (1 << 10, 1 << 31):
        cols = [list(d) for d in dims]
        cols[1][777] |= bad
        with pytest.raises(hl.ArgumentError, match="spark: index out of range"):
            _run(hl, ctx, cols, val, 10, point)
    assert _run(hl, ctx, dims, val, 10, point) == (E, v)
