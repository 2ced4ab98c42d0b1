"""The device radix sort (csrc/sort.hip) and the Lasso access counters (k_lasso_counters) on their own, through the
test-only entries lh_debug_sort_pairs / lh_debug_lasso_counters, against the numpy references of tests/sort_ref.py.

Integer in, integer out: every comparison is exact, outputs lie between guard words, and the inputs must read back
unchanged.  The shapes are the smallest that reach each branch of the sort - the wave and tile edges, the XCD tile remap of
the scatter pass (from 64 tiles, with and without a remainder), two and three tiles per thread of the histogram scan (above
256 and 512 tiles), first_bit != 0 with one and several passes, u64 keys of every width class, batches whose slabs differ in
pass count and digit width, the regrowth of the descriptor staging - and of the counters: the rank route, the partition
route with 2, 3, 5 and 7 partition bits, the column-by-column mode from 2^22 lookups, with and without keep_sorted /
keep_index.  A failure names the slab, its shape, the generator and the first differing index."""
import numpy as np
import pytest

import sort_ref as sr

pytestmark = pytest.mark.gpu

T = sr.TILE
SINGLE_NS = [1, 2, 63, 64, 65, 4095, 4096, 4097, 2 * T + 1,
             63 * T + 17,   # the last grid without the XCD remap
             64 * T,        # remap on, tiles % 8 == 0
             67 * T + 1,    # 68 tiles: remainder 4
             71 * T - 5,    # 71 tiles: remainder 7
             257 * T + 3,   # the scan gives two tiles per thread
             600 * T + 1]   # three tiles per thread, the last threads clamped
BITS = [1, 2, 5, 8, 9, 15, 16, 17, 24, 25, 32]
FIRST_BITS = [0, 3, 15]
BIT_PAIRS = [(b, f) for b in BITS for f in FIRST_BITS if b + f <= 32]
assert (8, 15) in BIT_PAIRS and (17, 15) in BIT_PAIRS and (32, 0) in BIT_PAIRS  # the counters' own use; sums of exactly 32


# ------------------------------------------------------------------ single u32 sorts
@pytest.mark.parametrize("bits", [8, 17, 32])
@pytest.mark.parametrize("n", SINGLE_NS)
def test_u32_sizes(ctx, n, bits):
    bad = sr.check_sort(ctx, "uniform", n, bits)
    assert not bad, sr.report(bad)


@pytest.mark.parametrize("bits,first_bit", BIT_PAIRS)
@pytest.mark.parametrize("n", [4097, 67 * T + 1])
def test_u32_bit_ranges(ctx, n, bits, first_bit):
    bad = sr.check_sort(ctx, "uniform", n, bits, first_bit)
    assert not bad, sr.report(bad)


@pytest.mark.parametrize("bits", [8, 17])
@pytest.mark.parametrize("n", [2 * T + 1, 64 * T])
@pytest.mark.parametrize("gen", sr.U32_GENERATORS)
def test_u32_generators(ctx, gen, n, bits):
    bad = sr.check_sort(ctx, gen, n, bits)
    assert not bad, sr.report(bad)


# ------------------------------------------------------------------ u64 sorts
@pytest.mark.parametrize("bits", [1, 8, 31, 32, 33, 37, 45, 63, 64])
@pytest.mark.parametrize("n", [1, 4097, 64 * T, 67 * T + 1])
@pytest.mark.parametrize("gen", sr.U64_GENERATORS)
def test_u64(ctx, gen, n, bits):
    bad = sr.check_sort(ctx, gen, n, bits, key_bytes=8)
    assert not bad, sr.report(bad)


# ------------------------------------------------------------------ batches
def _slab(gen, n, bits, first_bit=0, vals=True, seed=0):
    return sr.Slab(sr.make_keys(gen, n, bits, first_bit, 4, seed), bits, first_bit, sr.make_vals(n, seed) if vals else None, gen)


def test_batch_mixed_sizes_widths_and_first_bits(ctx):
    """slabs of one, two, three and four passes share every launch, with a different widest digit per pass"""
    shapes = [(0, 9, 0), (1, 4, 0), (100, 17, 3), (4096, 28, 0), (4097, 9, 15), (70000, 17, 0), (4097, 4, 28), (100, 28, 4),
              (70000, 4, 7), (0, 28, 0), (4096, 9, 23), (1, 17, 15), (70000, 28, 2), (100, 9, 0)]
    gens = ["uniform", "hot", "two", "equal"]
    slabs = [_slab(gens[i % 4], n, bits, fb, vals=i % 3 != 1, seed=i) for i, (n, bits, fb) in enumerate(shapes)]
    assert sorted({len(sr.plan_rb(s.bits)) for s in slabs}) == [1, 2, 3, 4]
    bad = sr.run_sort(ctx, slabs)[0]
    assert not bad, sr.report(bad)


def test_batch_adjacent_slabs_as_the_msm_lays_them_out(ctx):
    """37 slabs of 5000 pairs at offsets w n of ONE key and ONE value buffer: no output reaches into its neighbour"""
    slabs = [_slab(["uniform", "hot", "equal"][w % 3], 5000, 13, seed=w) for w in range(37)]
    bad = sr.run_sort(ctx, slabs, adjacent=True)[0]
    assert not bad, sr.report(bad)


def test_batch_remap_across_slab_boundaries(ctx):
    """24 slabs of 3 tiles + 7: 96 flattened tiles, the XCD remap spans the slab boundaries"""
    slabs = [_slab("uniform", 3 * T + 7, 17, seed=w) for w in range(24)]
    bad = sr.run_sort(ctx, slabs)[0]
    slabs = [_slab("uniform", 3 * T + 7, 8, 3, vals=False, seed=w) for w in range(23)]  # 92 tiles: remainder 4
    bad += sr.run_sort(ctx, slabs)[0]
    assert not bad, sr.report(bad)


def test_batch_descriptor_staging_regrows(ctx):
    """150 slab descriptors do not fit the first 16 KB of pinned staging; a small batch before and after"""
    small = [_slab("uniform", 300, 9, seed=w) for w in range(5)]
    many = [_slab("uniform", 300, [5, 9, 12][w % 3], w % 4, vals=w % 2 == 0, seed=100 + w) for w in range(150)]
    bad = sr.run_sort(ctx, small)[0] + sr.run_sort(ctx, many)[0] + sr.run_sort(ctx, small)[0]
    assert not bad, sr.report(bad)


def test_batch_twice_gives_identical_output(ctx):
    slabs = [_slab(g, n, bits, fb, seed=i) for i, (g, n, bits, fb) in enumerate(
        [("hot", 70000, 17, 0), ("two", 2 * T + 1, 9, 5), ("uniform", 4097, 28, 0), ("equal", 4096, 4, 0)])]
    bad1, k1, v1 = sr.run_sort(ctx, slabs)
    bad2, k2, v2 = sr.run_sort(ctx, slabs)
    assert not bad1 + bad2, sr.report(bad1 + bad2)
    for i in range(len(slabs)):
        assert (k1[i] == k2[i]).all() and (v1[i] == v2[i]).all(), slabs[i].describe(i)


# ------------------------------------------------------------------ argument errors: host checks, nothing is launched
def test_argument_errors(ctx):
    keys = sr.Guarded(ctx, [256, 256])
    k_in, k_out = keys.ptr(0), keys.ptr(1)

    def one(bits, first_bit, n=16, kin=k_in, kout=k_out, vout=k_out):
        return sr.slab_struct(kin, kout, None, vout, n, bits, first_bit)

    refused = {
        "bits = 0": sr.sort_call(ctx, 4, [one(0, 0)]),
        "first_bit + bits = 33": sr.sort_call(ctx, 4, [one(17, 16)]),
        "first_bit + bits = 33, one wide pass": sr.sort_call(ctx, 4, [one(1, 32)]),
        "bits = 33": sr.sort_call(ctx, 4, [one(33, 0)]),
        "first_bit + bits wraps": sr.sort_call(ctx, 4, [one(8, 0xFFFFFFFC)]),
        "key_bytes = 3": sr.sort_call(ctx, 3, [one(8, 0)]),
        "two u64 slabs": sr.sort_call(ctx, 8, [one(8, 0), one(8, 0)]),
        "u64 with first_bit": sr.sort_call(ctx, 8, [one(8, 3)]),
        "u64 bits = 65": sr.sort_call(ctx, 8, [one(65, 0)]),
        "null keys_in": sr.sort_call(ctx, 4, [one(8, 0, kin=None)]),
        "null keys_out": sr.sort_call(ctx, 4, [one(8, 0, kout=None)]),
        "null vals_out": sr.sort_call(ctx, 4, [one(8, 0, vout=None)]),
        "a bad slab behind a good one": sr.sort_call(ctx, 4, [one(8, 0), one(0, 0)]),
        "null slabs": ctx.lib.lh_debug_sort_pairs(ctx.h, 4, None, 1),
    }
    assert refused == {k: sr.LH_ERR_ARG for k in refused}, refused
    assert sr.sort_call(ctx, 4, []) == sr.LH_OK
    assert ctx.lib.lh_debug_sort_pairs(ctx.h, 4, None, 0) == sr.LH_OK
    assert sr.sort_call(ctx, 4, [one(8, 0, n=0, kin=None, kout=None, vout=None)] * 3) == sr.LH_OK  # only empty slabs
    assert sr.sort_call(ctx, 8, [one(64, 0, n=0, kin=None, kout=None, vout=None)]) == sr.LH_OK
    assert not keys.read().guard_failures("argument errors") and (keys.now == sr.GUARD).all()  # nothing was written
    bad = sr.check_sort(ctx, "uniform", 100, 8)  # ... and the ctx still sorts
    assert not bad, sr.report(bad)


# ------------------------------------------------------------------ the access counters
COUNTER_NS = [1, 5, 4097,
              (1 << 17) - 5, (1 << 17) + 4096,  # lg in the partition range, not powers of two: the rank route
              1 << 17, 1 << 18,                 # the partition route, 2 and 3 partition bits
              1 << 20]                          # 5 partition bits


def _check_counters(ctx, shape, cc, n, m):
    dims = [sr.make_addresses(shape, n, m, col=j) for j in range(cc)]
    want = [sr.counters_reference(d, m) for d in dims]
    return sr.run_counters(ctx, dims, m, True, want, shape) + sr.run_counters(ctx, dims, m, False, want, shape)


@pytest.mark.parametrize("m", [2, 256, 1 << 16])
@pytest.mark.parametrize("n", COUNTER_NS)
@pytest.mark.parametrize("cc", [1, 3])
def test_counters_sizes(ctx, cc, n, m):
    bad = _check_counters(ctx, "uniform", cc, n, m)
    assert not bad, sr.report(bad)


@pytest.mark.parametrize("m", [2, 1 << 16])
@pytest.mark.parametrize("cc,n", [(1, 5), (3, 4097), (1, (1 << 17) + 4096), (3, 1 << 17), (1, 1 << 18)])
@pytest.mark.parametrize("shape", ["one", "ascending", "hot"])
def test_counters_address_shapes(ctx, shape, cc, n, m):
    bad = _check_counters(ctx, shape, cc, n, m)
    assert not bad, sr.report(bad)


@pytest.mark.parametrize("cc", [1, 2])
def test_counters_column_by_column(ctx, cc):
    """from 2^22 lookups the columns go through the steps one after the other (7 partition bits)"""
    bad = _check_counters(ctx, "uniform", cc, 1 << 22, 1 << 16)
    assert not bad, sr.report(bad)


def test_counters_address_out_of_range(ctx):
    """an address equal to m: LH_ERR_ARG, the host's verdict on the `bad` flag after a normal run"""
    m, n = 256, 1000
    dim = sr.make_addresses("uniform", n, m)
    dim[617] = m
    din = sr.Guarded(ctx, [n], [dim])
    out = sr.Guarded(ctx, [n, m])
    assert sr.counters_call(ctx, [din.ptr(0)], n, m, [out.ptr(0)], [out.ptr(1)]) == sr.LH_ERR_ARG
    assert b"out of range" in ctx.lib.lh_last_error()
    assert not out.read().guard_failures("address out of range") and not din.read().unchanged_failures("address out of range")
    bad = _check_counters(ctx, "uniform", 1, n, m)  # ... and the ctx still counts
    assert not bad, sr.report(bad)
