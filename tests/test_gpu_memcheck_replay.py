"""GPU: lh_memcheck_replay - the read values of a RAM trace from its stores, an exclusive segmented scan over the operations
sorted by cell - against a plain replay (a loop over a dict).  Every test compares rv, wv and the final cells exactly.
The shapes of tests/test_gpu_memcheck_witness.py with and without an image; loads only, stores only, every operation on
its own cell; one store at either side of every wave, workgroup and tile boundary of a hot cell (whatever the tile, up to
4096 operations), alone and with a second cell interleaved; the refusals, and the ctx after them; the replay's output as
the witness kernels' input."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (10, 1), (10, 10), (11, 16), (13, 9), (16, 4)]
HOT_N = 14
HOT_AT = [0, 1, 63, 64, 65, 255, 256, 1023, 1024, 1025, 2047, 2048, 4095, 4096, 8191, 16383]


def _plain(addr, store, val, l, image):
    """-> (rv, wv, final): the rule itself"""
    mem = dict(enumerate(int(v) for v in image)) if image is not None else {}
    rv, wv = np.empty(len(addr), dtype=np.uint32), np.empty(len(addr), dtype=np.uint32)
    for i, (a, s, v) in enumerate(zip(addr.tolist(), store.tolist(), val.tolist())):
        rv[i] = mem.get(a, 0)
        if s:
            mem[a] = v
        wv[i] = mem.get(a, 0)
    return rv, wv, np.array([mem.get(a, 0) for a in range(1 << l)], dtype=np.uint32)


def _ops(n, l, seed, kind="mixed"):
    rng = np.random.default_rng(seed)
    N = 1 << n
    addr = rng.integers(0, 1 << l, size=N, dtype=np.uint64).astype(np.uint32)
    store = {"mixed": (rng.integers(0, 3, size=N) > 0), "loads": np.zeros(N, bool), "stores": np.ones(N, bool)}[kind]
    # (a store flag is any non-zero word; the word of a load is ignored, so it is not left zero)
    flag = np.where(store, rng.integers(1, 1 << 32, size=N, dtype=np.uint64), 0).astype(np.uint32)
    val = rng.integers(0, 1 << 32, size=N, dtype=np.uint64).astype(np.uint32)
    return addr, flag, val


def _image(l, seed):
    return np.random.default_rng(seed).integers(0, 1 << 32, size=1 << l, dtype=np.uint64).astype(np.uint32)


def _up(hl, ctx, a, vars_):
    return hl.U32Column(ctx.upload(np.ascontiguousarray(a, dtype=np.uint32).tobytes()), vars_)


def _run(hl, ctx, addr, store, val, l, image):
    n = len(addr).bit_length() - 1
    cols = [_up(hl, ctx, c, n) for c in (addr, store, val)]
    out = hl.memcheck_replay(ctx, *cols, l, image=None if image is None else _up(hl, ctx, image, l))
    return tuple(np.frombuffer(c.buf.read(), dtype=np.uint32) for c in out)


def _check(hl, ctx, addr, store, val, l, image, what=""):
    rv, wv, fin = _run(hl, ctx, addr, store, val, l, image)
    want = _plain(addr, store, val, l, image)
    assert np.array_equal(rv, want[0]), "rv " + what
    assert np.array_equal(wv, want[1]), "wv " + what
    assert np.array_equal(fin, want[2]), "final " + what


_CACHE = {}


def _case(n, l):
    if (n, l) not in _CACHE:
        _CACHE[(n, l)] = _ops(n, l, 7000 * n + 70 * l)
        for a in _CACHE[(n, l)]:
            a.setflags(write=False)
    return _CACHE[(n, l)]


@pytest.mark.parametrize("with_image", [False, True])
@pytest.mark.parametrize("n,l", SHAPES)
def test_replay_matches_the_plain_replay(hl, ctx, n, l, with_image):
    _check(hl, ctx, *_case(n, l), l, _image(l, n + l) if with_image else None)


@pytest.mark.parametrize("kind", ["loads", "stores"])
@pytest.mark.parametrize("n,l", [(1, 1), (13, 9), (16, 4)])
def test_loads_only_and_stores_only(hl, ctx, n, l, kind):
    addr, store, val = _ops(n, l, 31 * n + l, kind)
    for image in (None, _image(l, 3)):
        _check(hl, ctx, addr, store, val, l, image, kind)
    if kind == "loads":  # the memory ends as it began
        assert np.array_equal(_run(hl, ctx, addr, store, val, l, image)[2], image)


@pytest.mark.parametrize("n,l", [(1, 1), (10, 10), (11, 16), (13, 13)])
def test_every_operation_on_its_own_cell(hl, ctx, n, l):
    rng = np.random.default_rng(n * l)
    addr = rng.permutation(1 << l)[:1 << n].astype(np.uint32)
    _, store, val = _ops(n, l, 5 + n)
    for image in (None, _image(l, 4)):
        _check(hl, ctx, addr, store, val, l, image)


@pytest.mark.parametrize("cells", [1, 2])
@pytest.mark.parametrize("at", HOT_AT)
def test_one_store_on_a_hot_cell_at_every_boundary(hl, ctx, at, cells):
    """2^14 loads of cell 0 (cells = 2: of cells 0 and 1 in turn, so that segments end inside tiles) and ONE store at
    position `at`: the loads before it return the image's word, the loads behind it the stored one - through at least
    three store-free tiles for some `at`, whatever the tile size up to 4096"""
    N = 1 << HOT_N
    addr = (np.arange(N, dtype=np.uint32) & np.uint32(cells - 1))
    store, val = np.zeros(N, dtype=np.uint32), np.full(N, 0xBAD0BAD0, dtype=np.uint32)
    store[at], val[at] = 1, 0x5EED0000 + at
    for image in (np.array([0x11111111, 0x22222222], dtype=np.uint32), None):
        rv, wv, fin = _run(hl, ctx, addr, store, val, 1, image)
        word = [0, 0] if image is None else image.tolist()
        cell = at & (cells - 1)
        want = np.array(word, dtype=np.uint32)[addr]
        behind = (np.arange(N) > at) & (addr == cell)
        want[behind] = val[at]
        assert np.array_equal(rv, want), "rv"
        want_wv = want.copy()
        want_wv[at] = val[at]
        assert np.array_equal(wv, want_wv), "wv"
        word[cell] = int(val[at])
        assert fin.tolist() == word, "final"
        _check(hl, ctx, addr, store, val, 1, image)  # (and the loop over a dict says the same)


def test_refusals_and_the_ctx_afterwards(hl, ctx):
    n, l = 13, 9
    addr, store, val = _case(n, l)
    image = _image(l, 9)
    for at, a in ((5, 1 << l), ((1 << n) - 1, 1 << l), (77, (1 << 31) | int(addr[77])), (4096, 0xFFFFFFFF)):
        bad = addr.copy()
        bad[at] = a
        with pytest.raises(hl.InvalidSnark, match="Invalid memory trace"):
            _run(hl, ctx, bad, store, val, l, image)
        _check(hl, ctx, addr, store, val, l, image, "after a refusal")  # a second, valid call on the same ctx


def test_the_replay_feeds_the_witness_kernels(hl, ctx):
    n, l = 13, 9
    addr, store, val = _case(n, l)
    image = _image(l, 11)
    cols = [_up(hl, ctx, c, n) for c in (addr, store, val)]
    rv, wv, fin = hl.memcheck_replay(ctx, *cols, l, image=_up(hl, ctx, image, l))
    rt, fv, ft, m, bad = hl.memcheck_witness(ctx, cols[0], rv, wv, l, init=[int(v) for v in image])
    assert not bad and sum(m) == 1 << n
    assert np.array_equal(np.array(fv, dtype=np.uint32), np.frombuffer(fin.buf.read(), dtype=np.uint32))
