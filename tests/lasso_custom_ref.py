"""TEST INFRASTRUCTURE ONLY: caller-registered subtables on top of oracle/pyref/lasso.py, in the style of
tests/lasso_tables_ref.py (whose OR / EQ / LTU wrappers every other kind is delegated to).

A custom kind is a number >= 0x100 that names a list of 2^l values:
  subtable_entry(kind, m, l)      = values[m]
  subtable_mle_eval(kind, point)  = oracle.pyref.poly.evaluate(values, point)     (variable i = index bit i)
The kind is not absorbed into any transcript, so the oracle's proof does not depend on which number a table got: the golden
generator uses fixed numbers, the tests the kinds the library's registry handed out.

`installed(tables)` installs the wrappers for `tables` = {kind: values} and restores what was there before.
"""
import contextlib
import random
import zlib

import lasso_tables_ref as ltr
from oracle.pyref import lasso as o_lasso
from oracle.pyref.field import R_MOD as P
from oracle.pyref.poly import evaluate

CUSTOM_BASE = 0x100
EQ, LTU = ltr.SUBTABLE_EQ, ltr.SUBTABLE_LTU


@contextlib.contextmanager
def installed(tables):
    tables = {int(k): [int(v) for v in vals] for k, vals in tables.items()}
    assert all(k >= CUSTOM_BASE and len(v) >= 2 and len(v) & (len(v) - 1) == 0 for k, v in tables.items())

    def subtable_entry(kind, m, l):
        if kind in tables:
            assert len(tables[kind]) == 1 << l
            return tables[kind][m]
        return ltr.subtable_entry(kind, m, l)

    def subtable_mle_eval(kind, point):
        if kind in tables:
            assert len(tables[kind]) == 1 << len(point)
            return evaluate(tables[kind], point)
        return ltr.subtable_mle_eval(kind, point)

    before = o_lasso.subtable_entry, o_lasso.subtable_mle_eval
    o_lasso.subtable_entry, o_lasso.subtable_mle_eval = subtable_entry, subtable_mle_eval
    try:
        yield
    finally:
        o_lasso.subtable_entry, o_lasso.subtable_mle_eval = before


# ------------------------------------------------------------------ the named tables
def signed(v, h):
    return v - (1 << h) if v >> (h - 1) else v


def lts_values(l):
    """the top chunk of a signed comparison: (sx < sy) on the two's-complement l/2-bit halves of m = x || y"""
    h = l // 2
    return [int(signed(m >> h, h) < signed(m & ((1 << h) - 1), h)) for m in range(1 << l)]


def _rand_bits(seed, l, first):
    rng = random.Random(seed)
    vals = [rng.randrange(2) for _ in range(1 << l)]
    vals[0] = first
    if first == 0:
        vals[1] = 1  # (never the all-zero table)
    return vals


def _wide():
    rng = random.Random(0x71de)
    vals = [rng.randrange(1 << 32) for _ in range(16)]
    vals[0], vals[5], vals[15] = 0, (1 << 32) - 1, 1 << 31
    return vals


TABLES = {
    "rand1": _rand_bits(31, 3, 0),    # l = 3, one-bit values, T[0] = 0
    "rand1n": _rand_bits(32, 3, 1),   # the same with T[0] = 1
    "wide": _wide(),                  # l = 4, values up to 2^32 - 1, T[0] = 0
    "zero": [0] * 4,                  # l = 2, all zero
    "and8": [(m >> 4) & (m & 15) for m in range(256)],  # the AND subtable's own entries at l = 8
    "lts": lts_values(4),             # the signed top-chunk subtable at l = 4
}


def bits_of(values):
    return len(values).bit_length() - 1


# ------------------------------------------------------------------ the cases: (name, c, n, g) over one named table
# g "linear": a = sum_j 2^j E_j (one memory per chunk); "product": a = prod_j E_j
CASES = [("rand1", 2, 4, "linear"), ("rand1n", 2, 2, "product"), ("wide", 1, 5, "linear"), ("zero", 1, 3, "linear")]


def g_terms(c, g):
    return [(1 << j, (j,)) for j in range(c)] if g == "linear" else [(1, tuple(range(c)))]


def spec_of(name, c, g, kind):
    """the oracle's side of a table whose c memories (chunk j each) all name `kind` = the registered TABLES[name]"""
    return o_lasso.TableSpec(name, c, bits_of(TABLES[name]), [(j, kind) for j in range(c)], g_terms(c, g))


def table_of(hl, name, c, g, kind):
    return hl.LassoTable(c, bits_of(TABLES[name]), [(j, kind) for j in range(c)], [(co, list(f)) for co, f in g_terms(c, g)])


def less_than_signed_spec(c, l, kind):
    """less_than's shape (tests/lasso_tables_ref.py less_than_table) with the top chunk's LTU replaced by `kind` = lts_values(l)"""
    memories = [(j, LTU) for j in range(c - 1)] + [(c - 1, kind)] + [(j, EQ) for j in range(1, c)]
    return o_lasso.TableSpec("less_than_signed", c, l, memories,
                             [(1, (j,) + tuple(c + k - 1 for k in range(j + 1, c))) for j in range(c)])


def random_dims(tag, c, l, n):
    """chunk columns seeded by the case; every column holds 0, 2^l - 1 and a repeated index where it has the room"""
    rng = random.Random(zlib.crc32(repr((tag, c, l, n)).encode()))
    dims = [[rng.randrange(1 << l) for _ in range(1 << n)] for _ in range(c)]
    for d in dims:
        if len(d) >= 4:
            d[0], d[1], d[2] = 0, (1 << l) - 1, d[3]
    return dims


def comparison_dims(c, l, n):
    """lasso_tables_ref.random_dims's recipe: equal operands in a third of the lookups"""
    return ltr.random_dims("less_than_signed", c, l, n)


def signed_operands(dims, l):
    h = l // 2
    xs, ys = ltr.operands(dims, l)
    return [signed(x, len(dims) * h) for x in xs], [signed(y, len(dims) * h) for y in ys]
