"""GPU: the keyed field sum of Spartan (csrc/kernels_spartan.hip spartan_spmv through lh_debug_spartan_spmv) on its own,
exactly, against its restatement in big-integer arithmetic (spartan_ref.spmv), in both directions: out[s] = sum of
val[k] X[other[k]] over the entries with seg[k] = s.  The output buffers are filled with non-zero bytes before the launch
(hl.spartan_spmv does it): a segment without entries must come out zero.  2^14 entries are at least four tiles whatever the
tile size up to 4096 (spartan_ref.TILE): segments that end on every power-of-two tile boundary, one segment over every
tile, one entry per segment, almost every segment empty, a heavy segment among uniform ones with the input unsorted."""
import array
import random

import pytest

import logup_gkr_ref as lgr
import spartan_ref as spa
from oracle.pyref.field import R_MOD as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pp16(hl, ctx):
    """sixteen variables whose first fourteen secrets are `mid`'s"""
    rng = random.Random(lgr.MID_SRS_SEED + 1)
    return hl.MultilinearKzg.setup(ctx, lgr.mid_ss() + [rng.randrange(1, P) for _ in range(2)])


def _matrix(rng, n, seg, other, shuffle):
    """(seg, other, val) of 2^n entries; shuffled: the caller's order is not the sorted one"""
    N = 1 << n
    assert len(seg) == len(other) == N
    val = [rng.randrange(P) for _ in range(N)]
    if shuffle:
        order = list(range(N))
        rng.shuffle(order)
        seg, other, val = [seg[i] for i in order], [other[i] for i in order], [val[i] for i in order]
    return list(seg), list(other), val


def _check(hl, ctx, pp, rng, n, l, mats, transposed=True):
    """mats: three (seg, other, val).  As rows (direction 0 sums by seg, direction 1 by other) and, transposed, as columns"""
    M = 1 << l
    X = [rng.randrange(P) for _ in range(M)]
    X[rng.randrange(M)] = 0
    up = lambda col: hl.U32Column(ctx.upload(array.array("I", col).tobytes()), n)
    for flip in ((False, True) if transposed else (False,)):
        cols = [(up(o), up(s), hl.MultilinearPolynomial.new(ctx, v)) if flip else (up(s), up(o), hl.MultilinearPolynomial.new(ctx, v))
                for s, o, v in mats]
        with hl.r1cs_commit(ctx, pp, cols, l) as key:
            by_seg = hl.spartan_spmv(ctx, key, 1 if flip else 0, X)
            by_other = hl.spartan_spmv(ctx, key, 0 if flip else 1, X)
        for m, (s, o, v) in enumerate(mats):
            assert by_seg[m] == spa.spmv(s, o, v, X, M), ("by segment", m, flip)
            assert by_other[m] == spa.spmv(o, s, v, X, M), ("by the other index", m, flip)


def test_the_smallest(hl, ctx, pp16):
    rng = random.Random(1)
    mats = [_matrix(rng, 1, s, o, False) for s, o in (([0, 3], [1, 1]), ([2, 2], [0, 3]), ([3, 0], [2, 1]))]
    _check(hl, ctx, pp16, rng, 1, 2, mats)


def test_every_entry_in_one_segment(hl, ctx, pp16):
    n, l = 14, 10
    rng = random.Random(2)
    N, M = 1 << n, 1 << l
    mats = [_matrix(rng, n, [seg] * N, [rng.randrange(M) for _ in range(N)], False) for seg in (0, M - 1, 517)]
    _check(hl, ctx, pp16, rng, n, l, mats)


@pytest.mark.parametrize("shifts", [(8, 9, 10), (11, 12, 13)])
def test_segments_end_on_every_power_of_two_tile_boundary(hl, ctx, pp16, shifts):
    n, l = 14, 14
    rng = random.Random(3 + shifts[0])
    N, M = 1 << n, 1 << l
    # seg[k] = k >> s in the sorted stream; the keys are spread over the range so that empty segments lie between them
    mats = [_matrix(rng, n, [(k >> s) * 3 + 1 for k in range(N)], [rng.randrange(M) for _ in range(N)], s % 2 == 0) for s in shifts]
    assert all(max(m[0]) < M for m in mats)
    _check(hl, ctx, pp16, rng, n, l, mats)


def test_one_entry_per_segment(hl, ctx, pp16):
    n, l = 14, 14
    rng = random.Random(4)
    N, M = 1 << n, 1 << l
    perm = list(range(M))
    mats = []
    for _ in range(3):
        rng.shuffle(perm)
        mats.append(_matrix(rng, n, list(perm), [rng.randrange(M) for _ in range(N)], False))
    _check(hl, ctx, pp16, rng, n, l, mats)


def test_almost_every_segment_empty(hl, ctx, pp16):
    n, l = 10, 16
    rng = random.Random(5)
    N, M = 1 << n, 1 << l
    mats = [_matrix(rng, n, [rng.randrange(M) for _ in range(N)], [rng.randrange(M) for _ in range(N)], False) for _ in range(3)]
    mats[1] = _matrix(rng, n, [M - 1] * (N // 2) + [0] * (N // 2), mats[1][1], True)  # the two ends of the range
    _check(hl, ctx, pp16, rng, n, l, mats)


def test_a_heavy_segment_among_uniform_ones_unsorted_with_duplicates(hl, ctx, pp16):
    n, l = 14, 12
    rng = random.Random(6)
    N, M = 1 << n, 1 << l
    mats = []
    for heavy in (1 << (l - 1), 0, M - 1):
        seg = [heavy] * (N // 2) + [rng.randrange(M) for _ in range(N // 2)]
        other = [rng.randrange(M) for _ in range(N // 2)] * 2  # every (segment-mate) index twice: positions repeat
        mats.append(_matrix(rng, n, seg, other, True))
    _check(hl, ctx, pp16, rng, n, l, mats)


def test_three_matrices_of_different_structure_in_one_launch(hl, ctx, pp16):
    n, l = 13, 9
    rng = random.Random(7)
    N, M = 1 << n, 1 << l
    uniform = lambda: [rng.randrange(M) for _ in range(N)]
    mats = [_matrix(rng, n, [k >> 4 for k in range(N)], uniform(), True),  # every segment 16 entries: all closed inside a row
            _matrix(rng, n, [300] * N, uniform(), False),                  # one segment over every tile
            _matrix(rng, n, uniform(), [7] * N, True)]                     # uniform segments, one gathered element
    mats[2][2][:] = [0] * (N // 2) + mats[2][2][N // 2:]                   # (half of its values zero: padding entries)
    _check(hl, ctx, pp16, rng, n, l, mats)


def test_refusals(hl, ctx, pp16):
    rng = random.Random(8)
    up = lambda col: hl.U32Column(ctx.upload(array.array("I", col).tobytes()), 1)
    cols = [(up([0, 1]), up([1, 2]), hl.MultilinearPolynomial.new(ctx, [3, 4])) for _ in range(3)]
    key = hl.r1cs_commit(ctx, pp16, cols, 2)
    X = [rng.randrange(P) for _ in range(4)]
    with pytest.raises(hl.ArgumentError, match="direction"):
        hl.spartan_spmv(ctx, key, 2, X)
    with pytest.raises(hl.ArgumentError, match="2\\^dim_vars"):
        hl.spartan_spmv(ctx, key, 0, X[:3])
    assert hl.spartan_spmv(ctx, key, 0, X)[0] == [3 * X[1] % P, 4 * X[2] % P, 0, 0]
    key.free()
    with pytest.raises(hl.ArgumentError, match="freed"):
        hl.spartan_spmv(ctx, key, 0, X)
