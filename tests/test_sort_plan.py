"""The radix sort's pass plan (csrc/sort.hip rs_plan / rs_batch_bytes) through the host-only entry lh_debug_sort_plan, and
the numpy references of tests/sort_ref.py against the plain definitions.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import sort_ref as sr

NS = [1, 4096, 4097, 1 << 24]


@pytest.fixture(scope="module")
def plan(hl):
    from halo2_lasso_amd import _ffi
    lib = _ffi.load()

    def plan(n, bits, key_bytes):
        passes, rb, temp = C.c_uint(), (C.c_uint * 8)(*([99] * 8)), C.c_size_t()
        st = lib.lh_debug_sort_plan(n, bits, key_bytes, C.byref(passes), rb, C.byref(temp))
        assert st == sr.LH_OK, (n, bits, key_bytes, st)
        return passes.value, list(rb), temp.value

    return plan


@pytest.mark.parametrize("key_bytes", [4, 8])
def test_plan_of_every_width(plan, key_bytes):
    bad = []
    for bits in range(1, 8 * key_bytes + 1):
        for n in NS:
            passes, rb, _ = plan(n, bits, key_bytes)
            used = rb[:passes]
            ok = (passes == -(-bits // 8) and sum(used) == bits and all(1 <= r <= 8 for r in used)
                  and max(used) - min(used) <= 1 and used == sorted(used, reverse=True) and rb[passes:] == [0] * (8 - passes)
                  and used == sr.plan_rb(bits))
            if not ok:
                bad.append("key_bytes=%d bits=%d n=%d: passes=%d rb=%s" % (key_bytes, bits, n, passes, rb))
    assert not bad, sr.report(bad)


def test_17_bits_are_6_6_5(plan):
    assert plan(4097, 17, 4)[:2] == (3, [6, 6, 5, 0, 0, 0, 0, 0])
    assert plan(4097, 17, 8)[:2] == (3, [6, 6, 5, 0, 0, 0, 0, 0])


@pytest.mark.parametrize("key_bytes", [4, 8])
def test_bits_above_the_key_width_clamp(plan, key_bytes):
    width = 8 * key_bytes
    for bits in (width + 1, width + 7, 200):
        for n in NS:
            assert plan(n, bits, key_bytes) == plan(n, width, key_bytes), (bits, n)


@pytest.mark.parametrize("key_bytes", [4, 8])
def test_temp_bytes(plan, key_bytes):
    """monotone in n; room for the 256 ntiles + 256 histogram words, and for a second set of pairs from two passes on"""
    bad = []
    for bits in range(1, 8 * key_bytes + 1):
        prev = 0
        for n in [1, 2, 4095, 4096, 4097, 8192, 8193, 70000, 1 << 20, (1 << 20) + 1, 1 << 24]:
            passes, _, temp = plan(n, bits, key_bytes)
            ntiles = -(-n // sr.TILE)
            floor = 1024 * ntiles + 1024 + (n * (key_bytes + 4) if passes >= 2 else 0)
            if temp < floor or temp < prev:
                bad.append("key_bytes=%d bits=%d n=%d: temp_bytes=%d, floor %d, at the previous n %d" % (
                    key_bytes, bits, n, temp, floor, prev))
            prev = temp
    assert not bad, sr.report(bad)


def test_plan_argument_errors(hl):
    from halo2_lasso_amd import _ffi
    lib = _ffi.load()
    passes, rb, temp = C.c_uint(), (C.c_uint * 8)(), C.c_size_t()
    assert lib.lh_debug_sort_plan(10, 8, 3, C.byref(passes), rb, C.byref(temp)) == sr.LH_ERR_ARG
    assert lib.lh_debug_sort_plan(10, 8, 4, None, rb, C.byref(temp)) == sr.LH_ERR_ARG


# ------------------------------------------------------------------ the references themselves
def test_sort_reference_is_a_stable_sort_of_the_field():
    keys = np.array([0x35, 0x11, 0x25, 0x15, 0x21, 0x31], dtype=np.uint32)  # field = bits [4, 6): 3 1 2 1 2 3
    k, v = sr.sort_reference(keys, 2, 4)
    assert list(k) == [0x11, 0x15, 0x25, 0x21, 0x35, 0x31] and list(v) == [1, 3, 2, 4, 0, 5]
    vals = np.array([9, 8, 7, 6, 5, 0xFFFFFFFF], dtype=np.uint32)
    assert list(sr.sort_reference(keys, 2, 4, vals)[1]) == [8, 6, 7, 5, 9, 0xFFFFFFFF]
    k64 = np.array([(3 << 40) | 1, (1 << 40) | 2, (1 << 40) | 0], dtype=np.uint64)
    assert list(sr.sort_reference(k64, 64)[1]) == [2, 1, 0] and list(sr.sort_reference(k64, 32)[1]) == [2, 0, 1]


@pytest.mark.parametrize("shape", sr.ADDRESS_SHAPES)
@pytest.mark.parametrize("m", [2, 256])
def test_counters_reference_is_the_definition(shape, m):
    dim = sr.make_addresses(shape, 777, m)
    assert dim.max() < m
    read_ts, final_cts, keep_sorted, keep_index = sr.counters_reference(dim, m)
    plain_ts, plain_cts = sr.counters_reference_plain(dim, m)
    assert (read_ts == plain_ts).all() and (final_cts == plain_cts).all()
    assert (keep_sorted == dim[keep_index]).all() and (np.diff(keep_sorted.astype(np.int64)) >= 0).all()
    assert sorted(keep_index) == list(range(777))


@pytest.mark.parametrize("key_bytes,gens", [(4, sr.U32_GENERATORS), (8, sr.U64_GENERATORS)])
def test_generators(key_bytes, gens):
    """what the generators promise: the field shape, random bits outside it, every digit of every pass"""
    width = 8 * key_bytes
    for gen in gens:
        for bits, first_bit in [(8, 0), (17, 0), (width, 0)] + ([(8, 15), (17, 15)] if key_bytes == 4 else [(37, 0)]):
            n = 2 * 4096 + 1
            keys = sr.make_keys(gen, n, bits, first_bit, key_bytes)
            assert keys.dtype == sr._dtype(key_bytes) and len(keys) == n
            f = sr.field_of(keys, bits, first_bit)
            outside = keys.astype(np.uint64) & np.uint64(((1 << width) - 1) & ~(((1 << bits) - 1) << first_bit))
            what = (gen, bits, first_bit)
            if gen == "equal":
                assert len(np.unique(keys)) == 1, what
            if gen == "two":
                assert len(np.unique(f)) == 2, what
            if gen == "ascending":
                assert (np.diff(f.astype(np.float64)) >= 0).all() and f[-1] > f[0], what
            if gen == "descending":
                assert (np.diff(f.astype(np.float64)) <= 0).all() and f[-1] < f[0], what
            if gen == "hot":
                assert 0.85 * n < np.unique(f, return_counts=True)[1].max() < 0.95 * n, what
            if gen == "high_only":
                assert len(np.unique(keys & np.uint64(0xFFFFFFFF))) == 1 and len(np.unique(keys >> np.uint64(32))) > n // 2
            if gen == "low_only":
                assert len(np.unique(keys >> np.uint64(32))) == 1 and len(np.unique(keys & np.uint64(0xFFFFFFFF))) > n // 2
            if gen in ("uniform", "two", "hot", "ascending") and bits + first_bit < width - 4:
                assert len(np.unique(outside)) > 8, what  # the bits outside the field are not constant
    v = sr.make_vals(4097)
    assert 0 in v and 0xFFFFFFFF in v and sr.make_vals(1)[0] == 0xFFFFFFFF
