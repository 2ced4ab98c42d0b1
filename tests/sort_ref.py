"""Key generators, numpy references and guarded device buffers for the radix sort (csrc/sort.hip) and the Lasso access
counters (csrc/kernels_poly.hip k_lasso_counters), run on their own through the test-only entries lh_debug_sort_pairs and
lh_debug_lasso_counters (include/lasso_hip.h, "development / tests").

Both operations are integer in, integer out: every comparison is exact.  The sort reference is numpy's stable argsort of
the sorted key field, (key >> first_bit) & (2^bits - 1); whole keys travel with it, so the bits outside the field are
checked too.  The counters' reference is the plain definition: read_ts[i] = number of earlier lookups of dim[i],
final_cts[a] = number of lookups of a.

Every device buffer is a Guarded: its regions lie between guard words of a known pattern.  After a run the guards must
hold, the outputs must equal the reference, and the INPUT buffers must read back as they were uploaded (dev.hpp promises
that a sort preserves its inputs, and the MSM sorts slabs that sit next to each other in one allocation).

check_sort and check_counters return a list of failure lines (empty: passed), each naming the slab or column, n, bits,
first_bit, the generator and the first differing index; report() joins them as field_edges.report does.
"""
import ctypes as C
import zlib

import numpy as np

TILE = 4096        # pairs per workgroup of the sort (sort.hip RS_TILE)
GUARD_WORDS = 64   # u32 words between two regions and at both ends of a buffer
GUARD = 0x5AA5C33C
LH_OK, LH_ERR_ARG = 0, -8

U32_GENERATORS = ["uniform", "equal", "two", "ascending", "descending", "hot", "every_digit"]
U64_GENERATORS = ["uniform", "equal", "high_only", "low_only"]


def plan_rb(bits):
    """the digit widths of the passes (sort.hip rs_plan): ceil(bits / 8) passes, the bits split evenly, wider digits first"""
    passes = (bits + 7) // 8
    rb, left = [], bits
    for i in range(passes):
        rb.append((left + (passes - i) - 1) // (passes - i))
        left -= rb[-1]
    return rb


def _rng(*what):
    return np.random.default_rng(zlib.crc32(repr(what).encode()))


def _dtype(key_bytes):
    return {4: np.uint32, 8: np.uint64}[key_bytes]


def field_of(keys, bits, first_bit):
    """the sorted field of every key, as u64"""
    mask = np.uint64((1 << bits) - 1)
    return (keys.astype(np.uint64) >> np.uint64(first_bit)) & mask


def make_keys(gen, n, bits, first_bit=0, key_bytes=4, seed=0):
    """n keys of the generator `gen`: the generator shapes the sorted field, the bits outside it are random (except where
    the generator says otherwise), so a sort that looks at the wrong bits, or drops the others, shows"""
    width = 8 * key_bytes
    assert 1 <= bits and first_bit + bits <= width
    rng = _rng(gen, n, bits, first_bit, key_bytes, seed)
    full = (1 << width) - 1
    fmask = ((1 << bits) - 1) << first_bit

    def rand_words(count):
        return rng.integers(0, 1 << 63, size=count, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=count, dtype=np.uint64)

    noise = rand_words(n) & np.uint64(full & ~fmask)
    idx = np.arange(n, dtype=np.uint64)
    if gen == "uniform":
        field = rand_words(n) & np.uint64((1 << bits) - 1)
    elif gen == "equal":  # one key, n times: 4096 pairs of one digit in every tile and pass
        field = np.full(n, int(rand_words(1)[0]) & ((1 << bits) - 1), dtype=np.uint64)
        noise = np.full(n, int(rand_words(1)[0]) & (full & ~fmask), dtype=np.uint64)
    elif gen == "two":  # two distinct field values; the bits outside tell equal keys apart
        a = int(rand_words(1)[0]) & ((1 << bits) - 1)
        b = a ^ (1 << int(rng.integers(0, bits)))
        field = np.where(rng.integers(0, 2, size=n) == 1, np.uint64(a), np.uint64(b)).astype(np.uint64)
    elif gen in ("ascending", "descending"):  # non-decreasing over the whole field range (runs of equal keys when n > 2^bits)
        if bits + max(n - 1, 1).bit_length() <= 64:
            field = (idx << np.uint64(bits)) // np.uint64(max(n, 1))
        else:
            field = idx * np.uint64(((1 << bits) - 1) // max(n, 1))
        if gen == "descending":
            field = field[::-1].copy()
    elif gen == "hot":  # ~90 % of the pairs share one field value (hot in every pass), the rest are uniform
        h = int(rand_words(1)[0]) & ((1 << bits) - 1)
        field = np.where(rng.random(n) < 0.9, np.uint64(h), rand_words(n) & np.uint64((1 << bits) - 1)).astype(np.uint64)
    elif gen == "every_digit":  # every digit of every pass occurs (n >= 2^rb), in a shuffled order
        field = np.zeros(n, dtype=np.uint64)
        shift = 0
        for q, rb in enumerate(plan_rb(bits)):
            assert n >= 1 << rb, "every_digit needs n >= 2^rb"
            digit = (idx * np.uint64(2 * q + 1) + np.uint64(q)) & np.uint64((1 << rb) - 1)
            field |= digit << np.uint64(shift)
            shift += rb
        field = field[rng.permutation(n)]
        shift = 0
        for rb in plan_rb(bits):
            assert len(np.unique((field >> np.uint64(shift)) & np.uint64((1 << rb) - 1))) == 1 << rb
            shift += rb
    elif gen in ("high_only", "low_only"):  # u64: keys that differ only above / only below bit 32
        assert key_bytes == 8 and first_bit == 0
        w = rand_words(n)
        const = int(rand_words(1)[0])
        if gen == "high_only":
            keys = (w & np.uint64(0xFFFFFFFF00000000)) | np.uint64(const & 0xFFFFFFFF)
        else:
            keys = (w & np.uint64(0xFFFFFFFF)) | np.uint64(const & 0xFFFFFFFF00000000)
        return keys.astype(np.uint64)
    else:
        raise KeyError(gen)
    keys = (field << np.uint64(first_bit)) | noise
    return keys.astype(_dtype(key_bytes))


def make_vals(n, seed=0):
    """random u32 values that include 0 and 0xffffffff"""
    rng = _rng("vals", n, seed)
    v = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    if n >= 1:
        v[rng.integers(0, n)] = 0xFFFFFFFF
    if n >= 2:
        v[0 if v[0] != 0xFFFFFFFF else 1] = 0
    return v


class Slab:
    """one sort: keys (u32 or u64 array), vals (u32 array, or None: the values are the positions)"""

    def __init__(self, keys, bits, first_bit=0, vals=None, gen="?"):
        self.keys, self.bits, self.first_bit, self.vals, self.gen = keys, bits, first_bit, vals, gen
        self.n = len(keys)

    def describe(self, i):
        return "slab %d (n=%d = %d tiles%+d, bits=%d, first_bit=%d, %s keys, generator %s, values %s)" % (
            i, self.n, self.n // TILE, self.n % TILE, self.bits, self.first_bit, self.keys.dtype, self.gen,
            "given" if self.vals is not None else "= positions")

    def expected(self):
        order = np.argsort(field_of(self.keys, self.bits, self.first_bit), kind="stable")
        return self.keys[order], (order.astype(np.uint32) if self.vals is None else self.vals[order])


def sort_reference(keys, bits, first_bit=0, vals=None):
    return Slab(keys, bits, first_bit, vals).expected()


# ------------------------------------------------------------------ guarded device buffers
class Guarded:
    """One device allocation of u32 words: guard | region 0 | guard | region 1 | ... | guard.  With adjacent=True the
    regions follow each other with nothing in between (the MSM's slab layout) and the guards stand at both ends only.
    Regions start at even word offsets unless adjacent.  `init` gives the words of a region (an input); other regions
    are filled with the guard pattern, so a pair that was never written shows as a mismatch."""

    def __init__(self, ctx, sizes, init=None, adjacent=False):
        self.offsets, off = [], GUARD_WORDS
        for s in sizes:
            self.offsets.append(off)
            off += s if adjacent else ((s + 1) & ~1) + GUARD_WORDS
        self.sizes = list(sizes)
        self.total = off + (GUARD_WORDS if adjacent else 0)
        self.host = np.full(self.total, GUARD, dtype=np.uint32)
        self.payload = np.zeros(self.total, dtype=bool)
        for i, s in enumerate(sizes):
            self.payload[self.offsets[i]:self.offsets[i] + s] = True
            if init is not None and init[i] is not None:
                self.host[self.offsets[i]:self.offsets[i] + s] = init[i].view(np.uint32)
        self.buf = ctx.upload(self.host.tobytes())

    def ptr(self, i):
        return self.buf.ptr + 4 * self.offsets[i]

    def read(self):
        self.now = np.frombuffer(self.buf.read(), dtype=np.uint32)
        return self

    def region(self, i, dtype=np.uint32):
        return self.now[self.offsets[i]:self.offsets[i] + self.sizes[i]].view(dtype)

    def guard_failures(self, what):
        bad = np.flatnonzero(~self.payload & (self.now != GUARD))
        if not len(bad):
            return []
        w = int(bad[0])
        after = [i for i, o in enumerate(self.offsets) if o + self.sizes[i] <= w]
        return ["%s: %d guard words overwritten, first at word %d (%s), now 0x%08x" % (
            what, len(bad), w, "before region 0" if not after else "%d words after the end of region %d" % (
                w - self.offsets[after[-1]] - self.sizes[after[-1]], after[-1]), int(self.now[w]))]

    def unchanged_failures(self, what):
        bad = np.flatnonzero(self.now != self.host)
        return [] if not len(bad) else ["%s: %d input words changed, first at word %d" % (what, len(bad), int(bad[0]))]

    def free(self):
        self.buf.free()


def _first_diff(got, want):
    d = np.flatnonzero(got != want)
    return None if not len(d) else int(d[0])


# ------------------------------------------------------------------ the sort
def sort_call(ctx, key_bytes, slab_structs):
    """lh_debug_sort_pairs on a list of _ffi.lh_debug_sort_slab; returns the status"""
    from halo2_lasso_amd import _ffi
    arr = (_ffi.lh_debug_sort_slab * max(len(slab_structs), 1))(*slab_structs)
    return ctx.lib.lh_debug_sort_pairs(ctx.h, key_bytes, arr, len(slab_structs))


def slab_struct(keys_in, keys_out, vals_in, vals_out, n, bits, first_bit=0):
    from halo2_lasso_amd import _ffi
    return _ffi.lh_debug_sort_slab(keys_in, keys_out, vals_in, vals_out, n, bits, first_bit)


def run_sort(ctx, slabs, key_bytes=4, adjacent=False):
    """one lh_debug_sort_pairs call over `slabs` (a batch); returns (failure lines, output key arrays, output value arrays)"""
    kw = key_bytes // 4
    kin = Guarded(ctx, [s.n * kw for s in slabs], [s.keys for s in slabs], adjacent)
    vin = Guarded(ctx, [s.n for s in slabs], [s.vals for s in slabs], adjacent)
    kout = Guarded(ctx, [s.n * kw for s in slabs], None, adjacent)
    vout = Guarded(ctx, [s.n for s in slabs], None, adjacent)
    structs = [slab_struct(kin.ptr(i), kout.ptr(i), vin.ptr(i) if s.vals is not None else None, vout.ptr(i), s.n, s.bits,
                           s.first_bit) for i, s in enumerate(slabs)]
    st = sort_call(ctx, key_bytes, structs)
    what = "batch of %d" % len(slabs) if len(slabs) != 1 else slabs[0].describe(0)
    if st != LH_OK:
        return ["%s: lh_debug_sort_pairs returned %d: %s" % (what, st, ctx.lib.lh_last_error().decode())], [], []
    for g in (kin, vin, kout, vout):
        g.read()
    bad = kin.unchanged_failures(what + ", keys_in") + vin.unchanged_failures(what + ", vals_in")
    bad += kout.guard_failures(what + ", keys_out") + vout.guard_failures(what + ", vals_out")
    keys_out, vals_out = [], []
    for i, s in enumerate(slabs):
        want_k, want_v = s.expected()
        got_k, got_v = kout.region(i, _dtype(key_bytes)), vout.region(i)
        keys_out.append(got_k.copy()), vals_out.append(got_v.copy())
        d = _first_diff(got_k, want_k)
        if d is not None:
            bad.append("%s: keys differ at %d of %d positions, first at index %d (tile %d): got 0x%x, want 0x%x" % (
                s.describe(i), int((got_k != want_k).sum()), s.n, d, d // TILE, int(got_k[d]), int(want_k[d])))
        d = _first_diff(got_v, want_v)
        if d is not None:
            bad.append("%s: values differ at %d of %d positions, first at index %d (tile %d, key 0x%x): got %d, want %d%s" % (
                s.describe(i), int((got_v != want_v).sum()), s.n, d, d // TILE, int(want_k[d]), int(got_v[d]), int(want_v[d]),
                " - the keys are right: equal keys left their order (stability)" if _first_diff(got_k, want_k) is None else ""))
    for g in (kin, vin, kout, vout):
        g.free()
    return bad, keys_out, vals_out


def check_sort(ctx, gen, n, bits, first_bit=0, key_bytes=4, seed=0):
    """one single sort, once with values given and once with values = positions"""
    keys = make_keys(gen, n, bits, first_bit, key_bytes, seed)
    bad = []
    for vals in (make_vals(n, seed), None):
        bad += run_sort(ctx, [Slab(keys, bits, first_bit, vals, gen)], key_bytes)[0]
    return bad


# ------------------------------------------------------------------ the access counters
def counters_reference(dim, m):
    """(read_ts, final_cts, keep_sorted, keep_index) of one column of addresses below m"""
    n = len(dim)
    order = np.argsort(dim, kind="stable")
    s = dim[order]
    first = np.ones(n, dtype=bool)
    first[1:] = s[1:] != s[:-1]
    starts = np.flatnonzero(first)
    rank = np.arange(n, dtype=np.int64) - starts[np.cumsum(first) - 1]
    read_ts = np.empty(n, dtype=np.uint32)
    read_ts[order] = rank.astype(np.uint32)
    return read_ts, np.bincount(dim, minlength=m).astype(np.uint32), s, order.astype(np.uint32)


def counters_reference_plain(dim, m):
    """the definition itself, one lookup after the other (small n: checks counters_reference)"""
    seen, read_ts = [0] * m, []
    for a in dim:
        read_ts.append(seen[int(a)])
        seen[int(a)] += 1
    return np.array(read_ts, dtype=np.uint32), np.array(seen, dtype=np.uint32)


ADDRESS_SHAPES = ["uniform", "one", "ascending", "hot"]


def make_addresses(shape, n, m, col=0, seed=0):
    rng = _rng("addr", shape, n, m, col, seed)
    if shape == "uniform":
        a = rng.integers(0, m, size=n)
    elif shape == "one":  # every lookup at one address: the last, the first, the middle cell
        a = np.full(n, (m - 1, 0, m // 2)[col % 3])
    elif shape == "ascending":
        a = np.arange(n, dtype=np.uint64) * np.uint64(m) // np.uint64(max(n, 1))
    elif shape == "hot":
        a = np.where(rng.random(n) < 0.9, int(rng.integers(0, m)), rng.integers(0, m, size=n))
    else:
        raise KeyError(shape)
    return np.asarray(a).astype(np.uint32)


def counters_call(ctx, dims, n, m, read_ts, final_cts, keep_sorted=None, keep_index=None):
    """lh_debug_lasso_counters on lists of device pointers; returns the status"""
    def arr(ptrs):
        return None if ptrs is None else (C.c_void_p * len(ptrs))(*ptrs)
    return ctx.lib.lh_debug_lasso_counters(ctx.h, arr(dims), len(dims), n, m, arr(read_ts), arr(final_cts), arr(keep_sorted),
                                           arr(keep_index))


def run_counters(ctx, dims, m, keep, want=None, shape="?"):
    """one lh_debug_lasso_counters call over the columns `dims`; `want`: the columns' counters_reference, if at hand"""
    cc, n = len(dims), len(dims[0])
    din = Guarded(ctx, [n] * cc, dims)
    # regions: read_ts of every column, final_cts of every column, then keep_sorted and keep_index of every column
    out = Guarded(ctx, [n] * cc + [m] * cc + ([n] * (2 * cc) if keep else []))
    cols = range(cc)
    st = counters_call(ctx, [din.ptr(j) for j in cols], n, m, [out.ptr(j) for j in cols], [out.ptr(cc + j) for j in cols],
                       [out.ptr(2 * cc + j) for j in cols] if keep else None,
                       [out.ptr(3 * cc + j) for j in cols] if keep else None)
    what = "counters (%d columns, n=%d, m=%d, %s addresses, keep_sorted / keep_index %s)" % (
        cc, n, m, shape, "given" if keep else "null")
    if st != LH_OK:
        return ["%s: lh_debug_lasso_counters returned %d: %s" % (what, st, ctx.lib.lh_last_error().decode())]
    din.read(), out.read()
    bad = din.unchanged_failures(what + ", dims") + out.guard_failures(what + ", outputs")
    for j in cols:
        ref = want[j] if want is not None else counters_reference(dims[j], m)
        names = ["read_ts", "final_cts"] + (["keep_sorted", "keep_index"] if keep else [])
        for r, name in enumerate(names):
            got = out.region(r * cc + j)
            d = _first_diff(got, ref[r])
            if d is not None:
                bad.append("%s, column %d: %s differs at %d of %d positions, first at index %d: got %d, want %d" % (
                    what, j, name, int((got != ref[r]).sum()), len(got), d, int(got[d]), int(ref[r][d])))
    din.free(), out.free()
    return bad


def report(bad, limit=12):
    return "%d failures:\n%s" % (len(bad), "\n".join(bad[:limit]))
