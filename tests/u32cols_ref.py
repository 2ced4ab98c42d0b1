"""Big-integer references, input cases and guarded device runs for the kernels that work on 32-bit columns without their
field-element views (csrc/kernels_poly.hip, "small-valued columns"), run one operation at a time through the test-only
entry lh_debug_u32_columns (include/lasso_hip.h, "development / tests").

The references are written from what the operations are defined to compute (the comments above the kernels, repeated in
the header), over canonical integers mod r: plain Python integers, no Montgomery form, no limbs.  Every comparison is
exact.  Device results are brought to canonical form by lh_fr_to_repr (tables) or on the host (the few sums a call returns
in caller memory).

Inputs: a column is a numpy u32 array - its region on the device.  The first lens[k] words are the column; where the
column is shorter than the table the operation runs over, the region goes on with NON-ZERO filler words up to the table's
end, so a kernel that reads past the column's length gets a wrong sum and a correct one never sees them.  Field-element
tables are FrTables (canonical limbs); they reach the device through lh_fr_from_repr.  All device memory is a
sort_ref.Guarded: guard words around every region, outputs pre-filled with the guard pattern (an entry that was never
written shows), inputs read back unchanged.

cases(op, cus) lists the input cases of the GPU suite (tests/test_gpu_u32_columns.py) as keyword dictionaries of build();
tests/test_u32cols_ref_cpu.py walks the small ones on the CPU: the references against a textbook sum-check, and against the
MUTANTS at the end of this file - plausible wrong kernels, each of which at least one case must tell from the reference.

check() returns failure lines (empty: passed) that name the operation, the shape, the column and the first differing index.
"""
import ctypes as C
import functools
import zlib

import numpy as np

from sort_ref import GUARD, Guarded, LH_ERR_ARG, LH_OK, report  # noqa: F401  (report, LH_*: for the tests)

R_MOD = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
MONT = (1 << 256) % R_MOD              # R mod r: the stored (Montgomery) form of 1
MONT_INV = pow(MONT, -1, R_MOD)
# canonical values whose STORED form is 0, R mod r and r - 1
STORED_EDGES = (0, 1, (R_MOD - 1) * MONT_INV % R_MOD)

OPS = ("inner_products_small", "inner_products_small_half", "inner_products_small_quads", "inner_products_quads",
       "lincomb_mixed", "lincomb_fold_small", "lincomb_bind2", "sc_round_u32_bind2")  # index = the entry's op code
LCM_MAX_FR, LCM_MAX_SMALL, LCF_MAX, LCB_MAX = 8, 24, 24, 24  # csrc/dev.hpp
IPS_GROUP, IPQ_GROUP = 4, 2                                  # columns per launch (kernels_poly.hip)
PATTERNS = ("uniform", "ones", "zero", "sparse")
SCALARS = ("random", "zero", "one")


def _rng(*what):
    return np.random.default_rng(zlib.crc32(repr(what).encode()))


def pad4(n):
    return (n + 3) & ~3


# ------------------------------------------------------------------ field-element tables
class FrTable:
    """n canonical field elements as an (n, 4) array of u64 limbs, little endian; ints() gives them as Python integers"""

    def __init__(self, limbs):
        self.limbs = np.ascontiguousarray(limbs, dtype=np.uint64).reshape(-1, 4)
        self._ints = None

    @classmethod
    def from_ints(cls, xs):
        t = cls(np.frombuffer(b"".join(x.to_bytes(32, "little") for x in xs), dtype=np.uint64))
        t._ints = list(xs)
        return t

    def __len__(self):
        return len(self.limbs)

    def ints(self):
        if self._ints is None:
            b = self.limbs.tobytes()
            self._ints = [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]
        return self._ints


def fr_random(n, seed, edges=True):
    """n random elements; with `edges`, the three STORED_EDGES stand at the first, the middle and the last entry (n < 3: as
    many as fit, for every other seed; which ones depends on the seed)"""
    rng = _rng("fr", n, seed)
    limbs = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(n, 4), dtype=np.uint64)
    limbs[:, 3] = rng.integers(0, R_MOD >> 192, size=n, dtype=np.uint64)  # top limb below r's: the element is below r
    t = FrTable(limbs)
    s = zlib.crc32(repr(seed).encode())
    if edges and (n >= 3 or (n and s % 2 == 0)):
        for j, pos in enumerate(sorted({0, n // 2, n - 1})):
            t.limbs[pos] = FrTable.from_ints([STORED_EDGES[(j + s) % 3]]).limbs[0]
    return t


def scalar(kind, seed):
    return {"zero": 0, "one": 1}[kind] if kind != "random" else fr_random(1, ("scalar", seed), False).ints()[0]


def column(pattern, length, region, seed):
    """a region of `region` >= length words: `length` words of the pattern, then non-zero filler"""
    rng = _rng("col", pattern, length, region, seed)
    a = np.empty(region, dtype=np.uint32)
    if pattern == "uniform":
        a[:length] = rng.integers(0, 1 << 32, size=length, dtype=np.uint64).astype(np.uint32)
    elif pattern == "ones":
        a[:length] = 0xFFFFFFFF
    elif pattern == "zero":
        a[:length] = 0
    elif pattern == "sparse":
        a[:length] = (rng.random(length) < 0.125).astype(np.uint32)
    else:
        raise KeyError(pattern)
    a[length:] = (np.arange(length, region, dtype=np.uint32) & np.uint32(0xFFFF)) | np.uint32(0xF1110001)
    return a


# ------------------------------------------------------------------ eq tables (variable j is bit j of the index)
def eq_at(y, i):
    """eq(y, i) = prod_j (bit j of i ? y_j : 1 - y_j): the definition"""
    v = 1
    for j, yj in enumerate(y):
        v = v * (yj if (i >> j) & 1 else 1 - yj) % R_MOD
    return v


def eq_table(y, entries=None):
    """the first `entries` values of eq(y, .) (all 2^len(y) by default)"""
    t = [1]
    for yj in y:
        t = [v * (1 - yj) % R_MOD for v in t] + [v * yj % R_MOD for v in t]
    return t if entries is None else t[:entries]


@functools.lru_cache(maxsize=4)
def eq_frtable(y, entries):
    """eq_table(y, entries) of a tuple y as an FrTable (kept: the cases of one size share their point)"""
    return FrTable.from_ints(eq_table(y, entries))


def num_vars_for(entries):
    return max(entries - 1, 0).bit_length()


# ------------------------------------------------------------------ <weights, words>
def dot_plain(ws, words):
    return sum(w * int(v) for w, v in zip(ws, words)) % R_MOD


def dot(table, words):
    """<table[:len(words)], words> mod r with the products summed limb by limb in numpy (32-bit limb x 16-bit half word:
    below 2^48, 2^16 of them to a u64); the CPU suite holds it against dot_plain"""
    words = np.asarray(words)
    n = len(words)
    assert n <= len(table)
    w32 = table.limbs[:n].view(np.uint32).reshape(n, 8)
    lo, hi = [0] * 8, [0] * 8
    for at in range(0, n, 1 << 16):
        w = w32[at:at + (1 << 16)].astype(np.uint64)
        v = words[at:at + (1 << 16)].astype(np.uint64)
        sl = (w * (v & np.uint64(0xFFFF))[:, None]).sum(axis=0, dtype=np.uint64)
        sh = (w * (v >> np.uint64(16))[:, None]).sum(axis=0, dtype=np.uint64)
        for j in range(8):
            lo[j] += int(sl[j])
            hi[j] += int(sh[j])
    return sum((lo[j] + (hi[j] << 16)) << (32 * j) for j in range(8)) % R_MOD


# ------------------------------------------------------------------ cases
class Case:
    """the inputs of one call.  cols[k]: the region of column k (u32 array), lens[k]: the column's length in words;
    weights: the device table (weights / eq table) or None; w: the columns' host weights; frs / w_fr: lincomb_mixed's
    field-element tables; r0, r1: the scalars; y: the point whose eq table `weights` belongs to (or None)"""

    def __init__(self, op, shape, n, cols=(), lens=(), weights=None, w=(), frs=(), w_fr=(), r0=0, r1=0, y=None):
        self.op, self.shape, self.n = op, shape, n
        self.cols, self.lens, self.weights, self.w = list(cols), list(lens), weights, list(w)
        self.frs, self.w_fr, self.r0, self.r1, self.y = list(frs), list(w_fr), r0, r1, y

    def what(self):
        return "%s (%s)" % (self.op, self.shape)


def _pick(options, i):
    return options[i % len(options)]


def build(op, **kw):
    return globals()["_build_" + op](**kw)


def _build_inner_products_small(n, count, rot=0):
    cols = [column(_pick(PATTERNS, k + rot), n, pad4(n), (n, count, k)) for k in range(count)]
    return Case("inner_products_small", "n=%d, count=%d, patterns from %s" % (n, count, _pick(PATTERNS, rot)), n, cols,
                [n] * count, fr_random(n, (n, count, rot)))


def _build_inner_products_small_half(half, count, rot=0, y0="random"):
    y = [scalar(y0, half)] + fr_random(num_vars_for(half), ("y", half), False).ints()  # (one point per half and y0)
    cols = [column(_pick(PATTERNS, k + rot), 2 * half, pad4(2 * half), (half, count, k)) for k in range(count)]
    return Case("inner_products_small_half", "half=%d, count=%d, y0 %s, patterns from %s" % (
        half, count, y0, _pick(PATTERNS, rot)), half, cols, [2 * half] * count, eq_frtable(tuple(y[1:]), half), r0=y[0], y=y)


def _build_inner_products_small_quads(quads, pattern, e0="random"):
    col = column(pattern, 4 * quads, 4 * quads, (quads, pattern))
    y = None
    if e0 == "eq":  # E_0 of a sum-check at the point y: the eq table of y[1..]
        y = [scalar(_pick(SCALARS, PATTERNS.index(pattern)), (quads, pattern))]
        y += fr_random(num_vars_for(2 * quads), ("y", quads, pattern), False).ints()
        table = FrTable.from_ints(eq_table(y[1:], 2 * quads))
    else:
        table = fr_random(2 * quads, (quads, pattern))
    return Case("inner_products_small_quads", "quads=%d, %s column, e0 %s" % (quads, pattern, e0), quads, [col], [4 * quads],
                table, y=y)


def quad_lens(quads):
    return {"zero": 0, "four": 4, "short": 4 * (quads - 1), "full": 4 * quads, "long": 8 * quads}


def _build_inner_products_quads(quads, lens, rot=0):
    """lens: names of quad_lens(), one per column"""
    ln = [quad_lens(quads)[name] for name in lens]
    cols = [column(_pick(PATTERNS, k + rot), ln[k], max(ln[k], 4 * quads), (quads, tuple(lens), k)) for k in range(len(ln))]
    return Case("inner_products_quads", "quads=%d, lens %s, patterns from %s" % (quads, "/".join(lens), _pick(PATTERNS, rot)),
                quads, cols, ln, fr_random(quads, (quads, tuple(lens))))


def _build_lincomb_mixed(n, num_fr, num_sm, rot=0):
    names = ("zero", "one", "short", "full", "long")
    ln = [{"zero": 0, "one": 1, "short": n - 1, "full": n, "long": n + 5}[_pick(names, k + rot)] for k in range(num_sm)]
    cols = [column(_pick(PATTERNS, k + rot), ln[k], pad4(max(ln[k], n)), (n, num_fr, num_sm, k)) for k in range(num_sm)]
    return Case("lincomb_mixed", "n=%d, %d tables, %d columns of lengths %s" % (n, num_fr, num_sm, ln), n, cols, ln,
                w=fr_random(num_sm, ("wsm", n, num_fr, num_sm, rot)).ints(),
                frs=[fr_random(n, ("fr", n, num_fr, num_sm, k)) for k in range(num_fr)],
                w_fr=fr_random(num_fr, ("wfr", n, num_fr, num_sm, rot)).ints())


def _build_lincomb_fold_small(half, count, x="random", rot=0):
    options = (0, 1, half - 1, half, half + 1, 2 * half - 1, 2 * half)
    ln = [_pick(options, k + rot) for k in range(count)]
    cols = [column(_pick(PATTERNS, k + rot), ln[k], pad4(2 * half), (half, count, k)) for k in range(count)]
    return Case("lincomb_fold_small", "half=%d, count=%d, x %s, lengths %s" % (half, count, x, ln[:8]), half, cols, ln,
                w=fr_random(count, ("coef", half, count, rot)).ints(), r0=scalar(x, (half, count)))


def _build_lincomb_bind2(size, count, rot=0):
    entries = 2 * size
    options = (4 * entries, 0, 4 * (entries // 2), 8 * entries)  # full, empty, a short multiple of 4, longer than the table
    ln = [_pick(options, k + rot) for k in range(count)]
    # (four lengths and four patterns: the pattern moves on by one every four columns, so that each meets every length)
    cols = [column(_pick(PATTERNS, k + rot + 1 + (k + rot) // 4), ln[k], max(ln[k], 4 * entries), (size, count, k)) for k in range(count)]
    return Case("lincomb_bind2", "size=%d, count=%d, r0 %s, r1 %s, lengths %s" % (
        size, count, _pick(SCALARS, rot), _pick(SCALARS, rot // 3), ln[:8]), size, cols, ln,
        fr_random(size, ("eq", size, count)), w=fr_random(count, ("w", size, count, rot)).ints(),
        r0=scalar(_pick(SCALARS, rot), ("r0", size, count)), r1=scalar(_pick(SCALARS, rot // 3), ("r1", size, count)))


def _build_sc_round_u32_bind2(size, pattern, rot=0):
    col = column(pattern, 8 * size, 8 * size, (size, pattern))
    return Case("sc_round_u32_bind2", "size=%d, %s column, r0 %s, r1 %s" % (
        size, pattern, _pick(SCALARS, rot), _pick(SCALARS, rot // 3)), size, [col], [8 * size],
        fr_random(size, ("eq", size, pattern)),
        r0=scalar(_pick(SCALARS, rot), ("r0", size, pattern)), r1=scalar(_pick(SCALARS, rot // 3), ("r1", size, pattern)))


def stride_size(cus):
    """the first size whose 2 size bound entries exceed the grid cap of the two bind2 kernels (8 workgroups of 256 per CU),
    plus 256: every lane of the capped grid strides at least once and two workgroups' worth of lanes twice"""
    return 4 * 256 * cus + 1 + 256


BIND_SIZES = (1, 2, 64, 127, 128, 129, "stride")
# the keyword of build() that is the operation's size
SIZE_KEY = {"inner_products_small": "n", "inner_products_small_half": "half", "inner_products_small_quads": "quads",
            "inner_products_quads": "quads", "lincomb_mixed": "n", "lincomb_fold_small": "half", "lincomb_bind2": "size",
            "sc_round_u32_bind2": "size"}


def cases(op, cus=256, size=None):
    """the GPU suite's input cases of one operation as keyword dictionaries of build(op, ...); `size`: only those of one
    size (the operation's n / half / quads / size; "stride" stands for stride_size(cus))"""
    out = []
    if op == "inner_products_small":
        # 63 / 64 / 65: around a wave; 255 / 256 / 257: around a workgroup; 2^18: the 1024 x 256 grid cap exactly, beyond it
        # lanes stride.  count 1 .. 4: every launch_ips<G>; 5 = 4 + 1, 9 = 4 + 4 + 1: the partials buffer used again
        for i, n in enumerate((1, 63, 64, 65, 255, 256, 257, 1 << 18, (1 << 18) + 1, 3 * (1 << 18) + 77)):
            for count in (1, 2, 3, 4, 5, 9):
                if count <= 5 or n < (1 << 18):
                    out.append(dict(n=n, count=count, rot=i + count))
    elif op == "inner_products_small_half":
        for i, half in enumerate((1, 2, 64, 257, (1 << 18) + 1)):
            for count in (1, 2, 3, 5):
                out.append(dict(half=half, count=count, rot=i + count, y0=_pick(SCALARS, i)))
    elif op == "inner_products_small_quads":
        for quads in (1, 2, 63, 64, 65, 256, 257, 1 << 18, (1 << 18) + 1, (1 << 19) + 5):
            big = quads >= (1 << 18)
            for pattern in (PATTERNS[:2] if big else PATTERNS):
                out.append(dict(quads=quads, pattern=pattern, e0="random"))
                if not big:
                    out.append(dict(quads=quads, pattern=pattern, e0="eq"))
    elif op == "inner_products_quads":
        # launch groups of IPQ_GROUP = 2 columns.  1: every length alone; 2: both short (the launch covers `most` < quads),
        # and empty with longer-than-the-table; 3: full + long, then a lone short tail; 5: both short | short + full | lone long
        arrangements = [("zero",), ("four",), ("short",), ("full",), ("long",), ("four", "short"), ("zero", "long"),
                        ("full", "long", "short"), ("short", "zero", "four", "full", "long")]
        for i, quads in enumerate((1, 64, 65, 257, (1 << 18) + 1)):
            for j, lens in enumerate(arrangements):
                out.append(dict(quads=quads, lens=lens, rot=i + j))
    elif op == "lincomb_mixed":
        for i, n in enumerate((1, 255, 257)):
            for j, (num_fr, num_sm) in enumerate(((0, 0), (0, 1), (1, 0), (1, 2), (LCM_MAX_FR, LCM_MAX_SMALL))):
                for rot in range(5 if (num_fr, num_sm) in ((0, 1), (1, 2)) else 1):  # (every length in the first column)
                    out.append(dict(n=n, num_fr=num_fr, num_sm=num_sm, rot=rot + i + j))
        out.append(dict(n=(1 << 20) + 1, num_fr=1, num_sm=2, rot=2))  # strides the 4096-workgroup grid
    elif op == "lincomb_fold_small":
        for i, half in enumerate((1, 2, 255, 257)):
            for count in (1, 2, LCF_MAX):
                for rot in range(7 if count == 1 else 2):  # (one column: every length)
                    for x in SCALARS:
                        out.append(dict(half=half, count=count, x=x, rot=rot + i))
        out.append(dict(half=(1 << 20) + 1, count=2, x="random", rot=2))  # lengths half - 1 and half
    elif op == "lincomb_bind2":
        for i, s in enumerate(BIND_SIZES):
            for count in ((1, 3) if s == "stride" else (1, 2, 3, LCB_MAX)):
                for rot in range(1 if s == "stride" else (4 if count == 1 else 2)):
                    out.append(dict(size=s, count=count, rot=rot + i + 3 * count))
    elif op == "sc_round_u32_bind2":
        for i, s in enumerate(BIND_SIZES):
            for j, pattern in enumerate(PATTERNS[:2] if s == "stride" else PATTERNS):
                out.append(dict(size=s, pattern=pattern, rot=i + 2 * j))
    else:
        raise KeyError(op)
    key = SIZE_KEY[op]
    if size is not None:
        out = [kw for kw in out if kw[key] == size]
    for kw in out:
        if kw[key] == "stride":
            kw[key] = stride_size(cus)
    return out


def size_of(op, kw):
    return kw[SIZE_KEY[op]]


# ------------------------------------------------------------------ references
def _bound4(r0, r1):
    """the weights of entries 4i .. 4i+3 in entry i of a table bound with r0 (variable 0) and r1 (variable 1)"""
    return [(1 - r1) * (1 - r0) % R_MOD, (1 - r1) * r0 % R_MOD, r1 * (1 - r0) % R_MOD, r1 * r0 % R_MOD]


def _column_sum(c, upto):
    """[sum_k w_k col_k[i] for i < upto] as unreduced integers; entries from lens[k] on are zero"""
    acc = [0] * upto
    for k, w in enumerate(c.w):
        v = c.cols[k][:min(c.lens[k], upto)].tolist()
        acc[:len(v)] = [a + w * x for a, x in zip(acc, v)]
    return acc


def _round_sums(eq_level, table, lanes):
    return [sum(e * table[2 * b + x] for b, e in enumerate(eq_level)) % R_MOD for x in lanes]


def reference(c):
    """{"sums": what the call returns in caller memory, "table": what it leaves in d_out, "taken": whether it ran}"""
    out = {"sums": None, "table": None, "taken": True}
    n = c.n
    if c.op == "inner_products_small":
        out["sums"] = [dot(c.weights, col[:n]) for col in c.cols]
    elif c.op == "inner_products_small_half":  # <column, eq(y)> over the full table of 2 half entries
        full = eq_frtable(tuple(c.y), 2 * n)
        out["sums"] = [dot(full, col[:2 * n]) for col in c.cols]
    elif c.op == "inner_products_small_quads":
        col, e0 = c.cols[0], c.weights.ints()
        e1 = FrTable.from_ints([(e0[2 * q] + e0[2 * q + 1]) % R_MOD for q in range(n)])
        out["sums"] = [dot(c.weights, col[0:4 * n:2]), dot(c.weights, col[1:4 * n:2]), dot(e1, col[2:4 * n:4]), dot(e1, col[3:4 * n:4])]
    elif c.op == "inner_products_quads":
        out["table"] = [dot(c.weights, col[:min(ln, 4 * n)][t::4]) for col, ln in zip(c.cols, c.lens) for t in range(4)]
    elif c.op == "lincomb_mixed":
        acc = _column_sum(c, n)
        for w, t in zip(c.w_fr, c.frs):
            acc = [a + w * x for a, x in zip(acc, t.ints())]
        out["table"] = [a % R_MOD for a in acc]
    elif c.op == "lincomb_fold_small":
        if not 1 <= len(c.cols) <= LCF_MAX:
            out["taken"] = False
        else:
            g, x = _column_sum(c, 2 * n), c.r0
            out["table"] = [((1 - x) * g[i] + x * g[i + n]) % R_MOD for i in range(n)]
    elif c.op in ("lincomb_bind2", "sc_round_u32_bind2"):
        if c.op == "sc_round_u32_bind2":
            c = Case(c.op, c.shape, n, c.cols, c.lens, c.weights, [1], r0=c.r0, r1=c.r1)
        m, b4 = _column_sum(c, 8 * n), _bound4(c.r0, c.r1)
        out["table"] = [(b4[0] * m[4 * i] + b4[1] * m[4 * i + 1] + b4[2] * m[4 * i + 2] + b4[3] * m[4 * i + 3]) % R_MOD
                        for i in range(2 * n)]
        out["sums"] = _round_sums(c.weights.ints(), out["table"], (0, 1) if c.op == "lincomb_bind2" else (1,))
    else:
        raise KeyError(c.op)
    return out


def quads_identity(c, sums):
    """inner_products_small_quads with e0 = eq(y[1..]): (1 - y0) even + y0 odd must be <column, eq(y)>; failure lines"""
    y0, full = c.y[0], FrTable.from_ints(eq_table(c.y, 4 * c.n))
    got, want = ((1 - y0) * sums[0] + y0 * sums[1]) % R_MOD, dot(full, c.cols[0][:4 * c.n])
    return [] if got == want else ["%s: (1 - y0) even + y0 odd = 0x%x, <column, eq(y)> = 0x%x" % (c.what(), got, want)]


def closed_form_heavy(n):
    """inner_products_small over n entries, every weight STORED as r - 1 and every word 0xFFFFFFFF: one product.  With
    n = 8 * 2^18 every lane of the capped grid adds 8 terms of (r - 1)(2^32 - 1) > 2^285: its accumulator carries into limb 9."""
    c = Case("inner_products_small", "n=%d, every weight stored as r - 1, every word 0xFFFFFFFF" % n, n,
             [column("ones", n, n, "heavy")], [n], FrTable(np.tile(FrTable.from_ints([STORED_EDGES[2]]).limbs, (n, 1))))
    return c, {"sums": [n * 0xFFFFFFFF * STORED_EDGES[2] % R_MOD], "table": None, "taken": True}


# ------------------------------------------------------------------ device runs
def _fr_bytes(x):
    return (x % R_MOD * MONT % R_MOD).to_bytes(32, "little")


def _fr_struct(x):
    from halo2_lasso_amd import _ffi
    v = _ffi.lh_fr()
    C.memmove(C.byref(v), _fr_bytes(x), 32)
    return v


def _fr_array(xs):
    from halo2_lasso_amd import _ffi
    arr = (_ffi.lh_fr * max(len(xs), 1))()
    C.memmove(arr, b"".join(_fr_bytes(x) for x in xs), 32 * len(xs))
    return arr


def out_entries(c):
    """field elements the call writes to d_out"""
    return {"inner_products_quads": 4 * len(c.cols), "lincomb_mixed": c.n, "lincomb_fold_small": c.n,
            "lincomb_bind2": 2 * c.n, "sc_round_u32_bind2": 2 * c.n}.get(c.op, 0)


def host_sums(c):
    return {"inner_products_small": len(c.cols), "inner_products_small_half": len(c.cols), "inner_products_small_quads": 4,
            "lincomb_bind2": 2, "sc_round_u32_bind2": 1}.get(c.op, 0)


class Staged:
    """a case on the device: the columns, the field-element tables (in stored form) and the output, each a Guarded"""

    def __init__(self, ctx, c):
        from halo2_lasso_amd import _ffi
        self.ctx, self.c = ctx, c
        self.cols = Guarded(ctx, [len(r) for r in c.cols], c.cols)
        tables = ([c.weights] if c.weights is not None else []) + c.frs
        self.frs = Guarded(ctx, [8 * len(t) for t in tables])
        for i, t in enumerate(tables):
            if len(t):
                tmp = ctx.upload(t.limbs.tobytes())
                assert ctx.lib.lh_fr_from_repr(ctx.h, tmp.ptr, len(t), self.frs.ptr(i)) == LH_OK, ctx.lib.lh_last_error()
                tmp.free()
        self.frs.host = self.frs.read().now.copy()  # (the stored forms: what must read back unchanged)
        self.stage_bad = self.frs.guard_failures(c.what() + ", staging the field-element tables")
        self.out = Guarded(ctx, [8 * out_entries(c)])
        count = len(c.cols)
        self.keep = [(C.c_void_p * max(count, 1))(*[self.cols.ptr(k) for k in range(count)]),
                     (C.c_size_t * max(count, 1))(*c.lens), _fr_array(c.w),
                     (C.c_void_p * max(len(c.frs), 1))(*[self.frs.ptr(i + (c.weights is not None)) for i in range(len(c.frs))]),
                     _fr_array(c.w_fr), (_ffi.lh_fr * max(host_sums(c), 1))(), C.c_int(-1)]
        a = self.args = _ffi.lh_debug_u32_args()
        a.d_cols = C.cast(self.keep[0], C.POINTER(C.c_void_p))
        a.lens = C.cast(self.keep[1], C.POINTER(C.c_size_t))
        a.w = C.cast(self.keep[2], C.POINTER(_ffi.lh_fr))
        a.count = count
        a.d_weights = self.frs.ptr(0) if c.weights is not None else None
        a.n = c.n
        a.d_fr = C.cast(self.keep[3], C.POINTER(C.c_void_p))
        a.w_fr = C.cast(self.keep[4], C.POINTER(_ffi.lh_fr))
        a.num_fr = len(c.frs)
        a.r0, a.r1 = _fr_struct(c.r0), _fr_struct(c.r1)
        a.d_out = self.out.ptr(0)
        a.out_host = C.cast(self.keep[5], C.POINTER(_ffi.lh_fr))
        a.taken = C.pointer(self.keep[6])
        self.launched = False

    def launch(self):
        """one call of the entry; returns its status"""
        if self.launched:  # (again on the same buffers: the output starts from the guard pattern again)
            self.out.buf.write(self.out.host.tobytes())
            C.memset(self.keep[5], 0, C.sizeof(self.keep[5]))
        self.launched = True
        self.keep[6].value = -1
        return self.ctx.lib.lh_debug_u32_columns(self.ctx.h, OPS.index(self.c.op), C.byref(self.args))

    def results(self):
        """(failure lines of guards and inputs, {"sums", "table" (FrTable), "taken", "untouched": d_out still the guard pattern})"""
        from halo2_lasso_amd import fr_from_bytes
        ctx, c, what = self.ctx, self.c, self.c.what()
        self.cols.read(), self.frs.read(), self.out.read()
        bad = self.stage_bad + self.cols.unchanged_failures(what + ", columns") + self.frs.unchanged_failures(what + ", field-element tables")
        bad += self.out.guard_failures(what + ", d_out")
        got = {"sums": [fr_from_bytes(bytes(self.keep[5][i])) for i in range(host_sums(c))] if host_sums(c) else None,
               "table": None, "taken": self.keep[6].value != 0, "untouched": bool((self.out.region(0) == GUARD).all())}
        n = out_entries(c)
        if n and not got["untouched"]:
            tmp = ctx.alloc(32 * n)
            assert ctx.lib.lh_fr_to_repr(ctx.h, self.out.ptr(0), n, tmp.ptr) == LH_OK, ctx.lib.lh_last_error()
            got["table"] = FrTable(np.frombuffer(tmp.read(), dtype=np.uint64))
            tmp.free()
        return bad, got

    def free(self):
        for g in (self.cols, self.frs, self.out):
            g.free()


def _where(c, kind, i):
    if c.op == "inner_products_quads":
        return "column %d (length %d), S_%d" % (i // 4, c.lens[i // 4], i % 4)
    if kind == "sums":
        if c.op in ("inner_products_small", "inner_products_small_half"):
            return "column %d" % i
        if c.op == "inner_products_small_quads":
            return ("even", "odd", "S2", "S3")[i]
        return "q(%d)" % (i if c.op == "lincomb_bind2" else 1)
    return "entry %d" % i


def compare(c, got, want):
    """failure lines of one call's results against the reference"""
    what, bad = c.what(), []
    if got["taken"] != want["taken"]:
        return ["%s: taken = %s, want %s" % (what, got["taken"], want["taken"])]
    if not want["taken"]:
        return [] if got["untouched"] else ["%s: not taken, but d_out was written" % what]
    if want["sums"] is not None:
        diff = [i for i, (g, w) in enumerate(zip(got["sums"], want["sums"])) if g != w]
        if diff:
            i = diff[0]
            bad.append("%s: %d of %d sums differ, first %s: got 0x%x, want 0x%x" % (
                what, len(diff), len(want["sums"]), _where(c, "sums", i), got["sums"][i], want["sums"][i]))
    if want["table"] is not None:
        if got["table"] is None:
            return bad + ["%s: d_out was not written" % what]
        diff = np.flatnonzero((got["table"].limbs != FrTable.from_ints(want["table"]).limbs).any(axis=1))
        if len(diff):
            i = int(diff[0])
            bad.append("%s: %d of %d entries of d_out differ, first %s: got 0x%x, want 0x%x" % (
                what, len(diff), len(want["table"]), _where(c, "table", i), FrTable(got["table"].limbs[i]).ints()[0], want["table"][i]))
    return bad


def check(ctx, c, want=None):
    """one call of the case on the device against the reference (`want`: the reference's result, if at hand)"""
    s = Staged(ctx, c)
    try:
        st = s.launch()
        if st != LH_OK:
            return ["%s: lh_debug_u32_columns returned %d: %s" % (c.what(), st, ctx.lib.lh_last_error().decode())]
        bad, got = s.results()
        return bad + compare(c, got, want if want is not None else reference(c))
    finally:
        s.free()


def check_cases(ctx, op, cus, size=None):
    bad = []
    for kw in cases(op, cus, size):
        bad += check(ctx, build(op, **kw))
    return bad


# ------------------------------------------------------------------ mutants: plausible wrong kernels
# Each takes a Case of ITS operation and returns what reference() returns.  The CPU suite requires, for every mutant, a case
# of the GPU suite whose result differs from the reference's: the inputs can tell this bug from a correct kernel.
def mutant_yz_swapped(c):
    """inner_products_small_quads with the .y and .z words of every uint4 swapped"""
    col = c.cols[0][:4 * c.n].reshape(-1, 4)[:, [0, 2, 1, 3]].reshape(-1)
    return reference(Case(c.op, c.shape, c.n, [col], c.lens, c.weights, y=c.y))


def mutant_mask_dropped(c):
    """lincomb_mixed without `i < sm_len[k]`: a short column is read up to the table's end"""
    return reference(Case(c.op, c.shape, c.n, c.cols, [max(ln, c.n) for ln in c.lens], None, c.w, c.frs, c.w_fr))


def mutant_mask_le(c):
    """lincomb_fold_small with `i <= len[k]` and `i + half <= len[k]`: one word past a column's end is read"""
    return reference(Case(c.op, c.shape, c.n, c.cols, [min(ln + 1, len(col), 2 * c.n) for ln, col in zip(c.lens, c.cols)],
                          None, c.w, r0=c.r0))


def mutant_hi_limbs_dropped(c):
    """lincomb_mixed whose reduction takes the low 8 limbs of an entry's accumulator and drops limbs 8 and 9.  The
    accumulator is the integer sum_k (w_k R^2 mod r) col_k[i] (the weights arrive times R, in stored form)"""
    want = reference(c)
    pre = [w * MONT * MONT % R_MOD for w in c.w]
    fr = reference(Case(c.op, c.shape, c.n, [], [], None, [], c.frs, c.w_fr))["table"]
    table = []
    for i in range(c.n):
        t = sum(p * int(col[i]) for p, col, ln in zip(pre, c.cols, c.lens) if i < ln)
        table.append(((t & ((1 << 256) - 1)) * MONT_INV * MONT_INV + fr[i]) % R_MOD)
    return dict(want, table=table)


def mutant_e0_for_e1(c):
    """inner_products_small_quads with S2, S3 against E_0[q] instead of E_1[q] = E_0[2q] + E_0[2q + 1]"""
    want = reference(c)
    col = c.cols[0]
    return dict(want, sums=want["sums"][:2] + [dot(c.weights, col[2:4 * c.n:4]), dot(c.weights, col[3:4 * c.n:4])])


def mutant_q_lanes_swapped(c):
    """lincomb_bind2 with q(0) taken from the odd lanes and q(1) from the even ones"""
    want = reference(c)
    return dict(want, sums=want["sums"][::-1])


def mutant_tail_column_skipped(c):
    """inner_products_small that never launches the last group when it is a lone tail column (count = 4 g + 1): its sum
    stays zero"""
    want = reference(c)
    skip = len(c.cols) > IPS_GROUP and len(c.cols) % IPS_GROUP == 1
    return dict(want, sums=want["sums"][:-1] + [0] if skip else want["sums"])


def mutant_clamp_missing(c):
    """inner_products_quads without min(len / 4, quads): a column longer than the table is summed to ITS end, against
    whatever lies behind e1 (taken as ones here)"""
    n = max([c.n] + [ln // 4 for ln in c.lens])
    e1 = FrTable.from_ints(c.weights.ints() + [1] * (n - c.n))
    return dict(reference(c), table=[dot(e1, col[:ln][t::4]) for col, ln in zip(c.cols, c.lens) for t in range(4)])


MUTANTS = {
    "yz_swapped": ("inner_products_small_quads", mutant_yz_swapped),
    "mask_dropped": ("lincomb_mixed", mutant_mask_dropped),
    "mask_le": ("lincomb_fold_small", mutant_mask_le),
    "hi_limbs_dropped": ("lincomb_mixed", mutant_hi_limbs_dropped),
    "e0_for_e1": ("inner_products_small_quads", mutant_e0_for_e1),
    "q_lanes_swapped": ("lincomb_bind2", mutant_q_lanes_swapped),
    "tail_column_skipped": ("inner_products_small", mutant_tail_column_skipped),
    "clamp_missing": ("inner_products_quads", mutant_clamp_missing),
}
