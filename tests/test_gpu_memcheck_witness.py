"""GPU: the witness kernels of the memory-checking argument on their own (lh_debug_memcheck_witness: the stable sort by
cell, the pass over the sorted positions, the wave-aggregated histogram of the time differences) against a numpy
restatement, at the tile edges of the sort and leaf kernels - one tile, one tile per half, more cells than operations, a
hot cell - with and without an image, and the `bad` flag for every kind of invalid trace."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (10, 1), (10, 10), (11, 16), (13, 9), (16, 4)]


def _make_trace(n, l, seed, with_init):
    """a consistent trace: random cells, two operations in three are stores; -> (addr, rv, wv, init or None)"""
    rng = np.random.default_rng(seed)
    N, M = 1 << n, 1 << l
    init = rng.integers(0, 1 << 32, size=M, dtype=np.uint64).astype(np.uint32) if with_init else None
    addr = rng.integers(0, M, size=N, dtype=np.uint64).astype(np.uint32)
    store = rng.integers(0, 3, size=N) > 0
    words = rng.integers(0, 1 << 32, size=N, dtype=np.uint64).astype(np.uint32)
    mem = init.copy() if with_init else np.zeros(M, dtype=np.uint32)
    rv, wv = np.empty(N, dtype=np.uint32), np.empty(N, dtype=np.uint32)
    for i in range(N):
        a = addr[i]
        rv[i] = mem[a]
        if store[i]:
            mem[a] = words[i]
        wv[i] = mem[a]
    return addr, rv, wv, init


def _restate(addr, wv, init, l):
    """rt, fv, ft, m from the trace's addresses and written values alone (the reads are what the prover checks)"""
    N, M = len(addr), 1 << l
    order = np.argsort(addr, kind="stable")
    sa = addr[order]
    same = np.concatenate(([False], sa[1:] == sa[:-1]))
    rt = np.zeros(N, dtype=np.int64)
    rt[order[same]] = order[np.flatnonzero(same) - 1] + 1
    last = np.concatenate((sa[1:] != sa[:-1], [True]))
    fv = init.astype(np.int64) if init is not None else np.zeros(M, dtype=np.int64)
    ft = np.zeros(M, dtype=np.int64)
    fv[sa[last]] = wv[order[last]]
    ft[sa[last]] = order[last] + 1
    m = np.bincount(np.arange(N) - rt, minlength=N)
    return rt, fv, ft, m


_CACHE = {}


def _case(n, l, with_init):
    key = (n, l, with_init)
    if key not in _CACHE:
        addr, rv, wv, init = _make_trace(n, l, 1000 * n + 10 * l + with_init, with_init)
        for a in (addr, rv, wv):
            a.setflags(write=False)
        _CACHE[key] = (addr, rv, wv, init, _restate(addr, wv, init, l))
    return _CACHE[key]


def _run(hl, ctx, addr, rv, wv, l, init):
    n = len(addr).bit_length() - 1
    cols = [hl.U32Column(ctx.upload(np.ascontiguousarray(c, dtype=np.uint32).tobytes()), n) for c in (addr, rv, wv)]
    return hl.memcheck_witness(ctx, *cols, l, init=None if init is None else [int(v) for v in init])


@pytest.mark.parametrize("with_init", [False, True])
@pytest.mark.parametrize("n,l", SHAPES)
def test_witness_matches_the_restatement(hl, ctx, n, l, with_init):
    addr, rv, wv, init, (rt, fv, ft, m) = _case(n, l, with_init)
    got_rt, got_fv, got_ft, got_m, bad = _run(hl, ctx, addr, rv, wv, l, init)
    assert not bad
    assert np.array_equal(got_rt, rt) and np.array_equal(got_fv, fv) and np.array_equal(got_ft, ft)
    assert np.array_equal(got_m, m) and int(np.sum(got_m)) == 1 << n
    # the restatement against the rule itself: a read returns the last value written, or the image's word
    prev = np.where(rt > 0, wv[np.maximum(rt - 1, 0)], (init if init is not None else np.zeros(1 << l, np.uint32))[addr])
    assert np.array_equal(prev, rv)
    if l == 1 and n == 10:  # a hot memory: most differences are small
        assert m[:4].sum() > (1 << n) // 2


def test_one_hot_cell_and_distinct_cells(hl, ctx):
    """the histogram's two extremes: every difference 0 (one atomic address), and difference i exactly once"""
    n = 12
    N = 1 << n
    wv = np.arange(N, dtype=np.uint32) * np.uint32(2654435761)
    rv = np.concatenate(([0], wv[:-1])).astype(np.uint32)
    rt, fv, ft, m, bad = _run(hl, ctx, np.zeros(N, dtype=np.uint32), rv, wv, 3, None)
    assert not bad and rt == list(range(N)) and m == [N] + [0] * (N - 1)
    assert fv == [int(wv[-1])] + [0] * 7 and ft == [N] + [0] * 7
    addr = np.random.default_rng(5).permutation(1 << 13)[:N].astype(np.uint32)
    rt, fv, ft, m, bad = _run(hl, ctx, addr, np.zeros(N, dtype=np.uint32), wv, 13, None)
    assert not bad and not any(rt) and m == [1] * N
    want_ft = np.zeros(1 << 13, dtype=np.int64)
    want_ft[addr] = np.arange(N) + 1
    assert np.array_equal(ft, want_ft)


@pytest.mark.parametrize("n,l", [(1, 1), (13, 9), (16, 4)])
def test_bad_is_set_for_each_kind_of_invalid_trace(hl, ctx, n, l):
    addr, rv, wv, init, (rt, _, _, _) = _case(n, l, True)
    N = 1 << n
    first = int(np.flatnonzero(rt == 0)[0])  # a read of the image
    later = int(np.flatnonzero(rt > 0)[-1]) if (rt > 0).any() else None  # a read of an earlier write
    damaged = []
    for at in [first] + ([later] if later is not None else []):
        r = rv.copy()
        r[at] ^= np.uint32(1 << 31)
        damaged.append(("rv at %d" % at, addr, r, wv, init))
    if later is not None:  # the write that a later operation reads back
        w = wv.copy()
        w[int(rt[later]) - 1] ^= np.uint32(1)
        damaged.append(("wv before %d" % later, addr, rv, w, init))
    for name, a in (("addr = 2^l", 1 << l), ("addr = 2^l + cell", (1 << l) | int(addr[N - 1])), ("addr high bit", 1 << 31),
                    ("addr all ones", 0xFFFFFFFF)):
        ad = addr.copy()
        ad[N - 1] = a
        damaged.append((name, ad, rv, wv, init))
    changed = init.copy()
    changed[int(addr[first])] ^= np.uint32(2)
    damaged.append(("another image", addr, rv, wv, changed))
    if (init[addr[rt == 0]] != 0).any():
        damaged.append(("no image", addr, rv, wv, None))
    for name, a, r, w, image in damaged:
        assert _run(hl, ctx, a, r, w, l, image)[4], name
    assert not _run(hl, ctx, addr, rv, wv, l, init)[4]
