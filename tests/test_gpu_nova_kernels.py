"""GPU: the kernels of a Nova fold on their own (csrc/kernels_nova.hip through lh_debug_nova_spmv2, lh_debug_nova_cross_term
and lh_debug_nova_fold), exactly, against their restatement in big-integer arithmetic, with the outputs pre-filled with
non-zero bytes.  nova_spmv2 - the keyed field sum with two right-hand sides - at the shapes where the segmented sum can go
wrong, and against two lh_debug_spartan_spmv calls; nova_cross_term and nova_fold at l = 2, 10 and 14 (the last more than one
workgroup's stride), with E2 absent and present, u = 1 and full-width, r = 0, and operands whose stored limbs sit at the
field's carry edges (tests/field_edges.py)."""
import array
import random

import pytest

import field_edges as fe
import logup_gkr_ref as lgr
import spartan_ref as spa
from oracle.pyref.field import R_MOD as P

pytestmark = pytest.mark.gpu

R_INV = pow(1 << 256, -1, P)
EDGES = [s * R_INV % P for s in fe.stored_edges(P)]  # the field elements whose stored (Montgomery) limbs are the edge values


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


def _vectors(rng, M):
    X1, X2 = [rng.randrange(P) for _ in range(M)], [rng.randrange(P) for _ in range(M)]
    X1[rng.randrange(M)] = 0
    for i, e in enumerate(EDGES[:M // 2]):  # carry edges among the gathered operands
        X2[(7 * i + 1) % M] = e
    return X1, X2


def _check(hl, ctx, pp, rng, n, l, mats):
    """mats: three (seg, other, val); both directions; X1 != X2, X1 = X2 (one device vector) and X2 = 0"""
    M = 1 << l
    X1, X2 = _vectors(rng, M)
    up = lambda col: hl.U32Column(ctx.upload(array.array("I", col).tobytes()), n)
    cols = [(up(s), up(o), hl.MultilinearPolynomial.new(ctx, v)) for s, o, v in mats]
    with hl.r1cs_commit(ctx, pp, cols, l) as key:
        for direction in (0, 1):
            want1 = [spa.spmv(*((s, o) if direction == 0 else (o, s)), v, X1, M) for s, o, v in mats]
            want2 = [spa.spmv(*((s, o) if direction == 0 else (o, s)), v, X2, M) for s, o, v in mats]
            got1, got2 = hl.nova_spmv2(ctx, key, direction, X1, X2)
            assert got1 == want1 and got2 == want2, ("two sides", direction)
            # ... which two launches of the one-sided kernel give too
            assert hl.spartan_spmv(ctx, key, direction, X1) == got1 and hl.spartan_spmv(ctx, key, direction, X2) == got2
            same1, same2 = hl.nova_spmv2(ctx, key, direction, X1, X1)
            assert same1 == want1 and same2 == want1, ("X1 = X2", direction)
            zero1, zero2 = hl.nova_spmv2(ctx, key, direction, X2, [0] * M)
            assert zero1 == want2 and zero2 == [[0] * M] * 3, ("X2 = 0", direction)


# ------------------------------------------------------------------ nova_spmv2
def test_spmv2_the_smallest(hl, ctx, pp16):
    rng = random.Random(1)
    mats = [_matrix(rng, 1, s, o, False) for s, o in (([0, 3], [1, 1]), ([2, 2], [0, 3]), ([3, 0], [2, 1]))]
    _check(hl, ctx, pp16, rng, 1, 2, mats)


def test_spmv2_a_partial_tile(hl, ctx, pp16):
    n, l = 5, 3
    rng = random.Random(2)
    N, M = 1 << n, 1 << l
    mats = [_matrix(rng, n, [rng.randrange(M) for _ in range(N)], [rng.randrange(M) for _ in range(N)], True) for _ in range(3)]
    _check(hl, ctx, pp16, rng, n, l, mats)


def test_spmv2_every_entry_in_one_segment(hl, ctx, pp16):
    n, l = 14, 10  # eight tiles of 2048: the one segment crosses them all
    rng = random.Random(3)
    N, M = 1 << n, 1 << l
    mats = [_matrix(rng, n, [seg] * N, [rng.randrange(M) for _ in range(N)], False) for seg in (0, M - 1, 517)]
    _check(hl, ctx, pp16, rng, n, l, mats)


@pytest.mark.parametrize("shifts", [(5, 6, 5), (11, 12, 11)])
def test_spmv2_segments_end_on_wave_row_and_tile_boundaries(hl, ctx, pp16, shifts):
    n, l = 14, 14
    rng = random.Random(4 + shifts[0])
    N, M = 1 << n, 1 << l
    # seg[k] = (k >> s) 3 + 1 in the sorted stream: 32 and 64 entries (half a wave row, a wave row), 2048 and 4096 (a tile, two)
    mats = [_matrix(rng, n, [(k >> s) * 3 + 1 for k in range(N)], [rng.randrange(M) for _ in range(N)], i == 1) for i, s in enumerate(shifts)]
    assert all(max(m[0]) < M for m in mats)
    _check(hl, ctx, pp16, rng, n, l, mats)


def test_spmv2_one_entry_per_segment(hl, ctx, pp16):
    n, l = 14, 14
    rng = random.Random(5)
    N, M = 1 << n, 1 << l
    perm = list(range(M))
    mats = []
    for _ in range(3):
        rng.shuffle(perm)
        mats.append(_matrix(rng, n, list(perm), [rng.randrange(M) for _ in range(N)], False))
    _check(hl, ctx, pp16, rng, n, l, mats)


def test_spmv2_three_matrices_of_different_structure_in_one_launch(hl, ctx, pp16):
    n, l = 13, 9
    rng = random.Random(6)
    N, M = 1 << n, 1 << l
    uniform = lambda: [rng.randrange(M) for _ in range(N)]
    mats = [_matrix(rng, n, [k >> 4 for k in range(N)], uniform(), True),  # every segment 16 entries: all closed inside a row
            _matrix(rng, n, [300] * N, uniform(), False),                  # one segment over every tile
            _matrix(rng, n, uniform(), [7] * N, True)]                     # uniform segments, one gathered element
    mats[2][2][:] = [0] * (N // 2) + mats[2][2][N // 2:]                   # (half of its values zero: padding entries)
    _check(hl, ctx, pp16, rng, n, l, mats)


def test_spmv2_refusals(hl, ctx, pp16):
    rng = random.Random(7)
    up = lambda col: hl.U32Column(ctx.upload(array.array("I", col).tobytes()), 1)
    cols = [(up([0, 1]), up([1, 2]), hl.MultilinearPolynomial.new(ctx, [3, 4])) for _ in range(3)]
    key = hl.r1cs_commit(ctx, pp16, cols, 2)
    X = [rng.randrange(P) for _ in range(4)]
    with pytest.raises(hl.ArgumentError, match="direction"):
        hl.nova_spmv2(ctx, key, 2, X, X)
    with pytest.raises(hl.ArgumentError, match="2\\^dim_vars"):
        hl.nova_spmv2(ctx, key, 0, X, X[:3])
    assert hl.nova_spmv2(ctx, key, 0, X, X)[1][0] == [3 * X[1] % P, 4 * X[2] % P, 0, 0]
    key.free()
    with pytest.raises(hl.ArgumentError, match="freed"):
        hl.nova_spmv2(ctx, key, 0, X, X)


# ------------------------------------------------------------------ nova_cross_term and nova_fold
def _column(rng, M, k):
    """M field elements: random, the carry edges from position k on, zeros"""
    col = [rng.randrange(P) for _ in range(M)]
    for i, e in enumerate(EDGES):
        col[(k + i) % M] = e
    col[(k + 3 * len(EDGES)) % M] = 0
    return col


def _cross_term(mz1, mz2, u1, u2, e1, e2):
    M = len(mz1[0])
    T = [(mz1[0][i] * mz2[1][i] + mz2[0][i] * mz1[1][i] - u1 * mz2[2][i] - u2 * mz1[2][i]) % P for i in range(M)]
    fails = lambda mz, u, e: sum(1 for i in range(M) if (mz[0][i] * mz[1][i] - u * mz[2][i] - (e[i] if e is not None else 0)) % P)
    return T, [fails(mz1, u1, e1), fails(mz2, u2, e2)]


@pytest.mark.parametrize("l", [2, 10, 14])
@pytest.mark.parametrize("wide_u", [False, True])
def test_cross_term(hl, ctx, l, wide_u):
    rng = random.Random(100 + l + 50 * wide_u)
    M = 1 << l
    u1, u2 = (rng.randrange(P), P - 1) if wide_u else (1, 1)
    mz1, mz2 = [_column(rng, M, 3 * k) for k in range(3)], [_column(rng, M, 5 * k + 1) for k in range(3)]
    # input 1 with the error vector that makes every row hold, but two; input 2 fresh: rows fail as they come
    e1 = [(mz1[0][i] * mz1[1][i] - u1 * mz1[2][i]) % P for i in range(M)]
    for i in (0, M - 1):
        e1[i] = (e1[i] + 1) % P
    for e2 in (None, _column(rng, M, 2)) if l < 14 else (_column(rng, M, 2),):  # (the largest shape: once)
        T, bad = hl.nova_cross_term(ctx, l, mz1, mz2, e1, e2, u1, u2)
        want_T, want_bad = _cross_term(mz1, mz2, u1, u2, e1, e2)
        assert T == want_T and bad == want_bad and bad[0] == (2 if M > 1 else 1) and bad[1] >= M - 2 * len(EDGES) - 2
    # both hold: no row counted; E1 absent
    c2 = [(mz2[0][i] * mz2[1][i] % P) * pow(u2, -1, P) % P for i in range(M)]
    e1[0], e1[M - 1] = (e1[0] - 1) % P, (e1[M - 1] - 1) % P
    T, bad = hl.nova_cross_term(ctx, l, mz1, [mz2[0], mz2[1], c2], e1, None, u1, u2)
    assert (T, bad) == _cross_term(mz1, [mz2[0], mz2[1], c2], u1, u2, e1, None) and bad == [0, 0]
    if l == 14:
        return
    T, bad = hl.nova_cross_term(ctx, l, [mz2[0], mz2[1], c2], mz1, None, e1, u2, u1)
    assert (T, bad) == _cross_term([mz2[0], mz2[1], c2], mz1, u2, u1, None, e1) and bad == [0, 0]


@pytest.mark.parametrize("l", [2, 10, 14])
def test_fold_vectors(hl, ctx, l):
    rng = random.Random(200 + l)
    M, half = 1 << l, 1 << (l - 1)
    w1, w2 = _column(rng, M, 0)[:half], _column(rng, M, 1)[:half]
    e1, t, e2 = _column(rng, M, 2), _column(rng, M, 4), _column(rng, M, 6)
    # (the largest shape: one challenge, both vectors present and both absent)
    for r in (0, 1, P - 1, rng.randrange(P), EDGES[0]) if l < 14 else (rng.randrange(P),):
        r2 = r * r % P
        for a, b in ((e1, e2), (e1, None), (None, e2), (None, None)) if l < 14 else ((e1, e2), (None, None)):
            want_w = [(x + r * y) % P for x, y in zip(w1, w2)]
            want_e = [((a[i] if a else 0) + r * t[i] + (r2 * b[i] if b else 0)) % P for i in range(M)]
            assert hl.nova_fold_vectors(ctx, l, w1, w2, a, t, b, r) == (want_w, want_e), (r, a is None, b is None)
            if a is not None:  # the outputs are input 1's buffers
                assert hl.nova_fold_vectors(ctx, l, w1, w2, a, t, b, r, in_place=True) == (want_w, want_e), (r, "in place")
