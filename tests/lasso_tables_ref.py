"""TEST INFRASTRUCTURE ONLY: the OR / EQ / LTU subtables on top of oracle/pyref/lasso.py, which knows IDENTITY, AND and XOR.

The oracle resolves `subtable_entry` and `subtable_mle_eval` as module globals at call time (oracle/pyref/hyperplonk.py calls
them as `lasso.subtable_entry`), so wrappers installed on the module extend it without touching it: every old kind is
delegated to the original function.  `installed()` is the context manager behind the tests' fixture: it restores the
originals afterwards.

Index m = x || y with y in the low h = l/2 bits.  MLEs with variable i = index bit i, y_i = point[i], x_i = point[h + i]:
  OR   sum_i 2^i (x_i + y_i - x_i y_i)
  EQ   prod_i e_i,  e_i = x_i y_i + (1 - x_i)(1 - y_i)
  LTU  sum_i (1 - x_i) y_i prod_{k > i} e_k        (the high bits decide first)
"""
import contextlib

from oracle.pyref import lasso as o_lasso
from oracle.pyref.field import R_MOD as P

SUBTABLE_OR, SUBTABLE_EQ, SUBTABLE_LTU = 3, 4, 5
NEW_KINDS = (SUBTABLE_OR, SUBTABLE_EQ, SUBTABLE_LTU)

_ORIG_ENTRY, _ORIG_MLE = o_lasso.subtable_entry, o_lasso.subtable_mle_eval


def _halves(m, l):
    h = l // 2
    return m >> h, m & ((1 << h) - 1)


def or_entry(m, l):
    x, y = _halves(m, l)
    return x | y


def eq_entry(m, l):
    x, y = _halves(m, l)
    return int(x == y)


def ltu_entry(m, l):
    x, y = _halves(m, l)
    return int(x < y)


def or_mle(point):
    h = len(point) // 2
    return sum((point[h + i] + point[i] - point[h + i] * point[i]) << i for i in range(h)) % P


def _e(point, i):
    h = len(point) // 2
    x, y = point[h + i], point[i]
    return (x * y + (1 - x) * (1 - y)) % P


def eq_mle(point):
    acc = 1
    for i in range(len(point) // 2):
        acc = acc * _e(point, i) % P
    return acc


def ltu_mle(point):
    h = len(point) // 2
    acc, above = 0, 1  # above: prod of e_k over the bits above i
    for i in reversed(range(h)):
        acc = (acc + (1 - point[h + i]) * point[i] % P * above) % P
        above = above * _e(point, i) % P
    return acc


ENTRY = {SUBTABLE_OR: or_entry, SUBTABLE_EQ: eq_entry, SUBTABLE_LTU: ltu_entry}
MLE = {SUBTABLE_OR: or_mle, SUBTABLE_EQ: eq_mle, SUBTABLE_LTU: ltu_mle}


def subtable_entry(kind, m, l):
    return ENTRY[kind](m, l) if kind in ENTRY else _ORIG_ENTRY(kind, m, l)


def subtable_mle_eval(kind, point):
    return MLE[kind](point) if kind in MLE else _ORIG_MLE(kind, point)


@contextlib.contextmanager
def installed():
    o_lasso.subtable_entry, o_lasso.subtable_mle_eval = subtable_entry, subtable_mle_eval
    try:
        yield
    finally:
        o_lasso.subtable_entry, o_lasso.subtable_mle_eval = _ORIG_ENTRY, _ORIG_MLE


# ------------------------------------------------------------------ table specs (the oracle's side of hl.LassoTable.*)
def or_table(c, l):
    return o_lasso.TableSpec("or", c, l, [(j, SUBTABLE_OR) for j in range(c)], [(1 << (l // 2 * j), (j,)) for j in range(c)])


def equal_table(c, l):
    return o_lasso.TableSpec("equal", c, l, [(j, SUBTABLE_EQ) for j in range(c)], [(1, tuple(range(c)))])


def less_than_table(c, l):
    memories = [(j, SUBTABLE_LTU) for j in range(c)] + [(j, SUBTABLE_EQ) for j in range(1, c)]
    return o_lasso.TableSpec("less_than", c, l, memories,
                             [(1, (j,) + tuple(c + k - 1 for k in range(j + 1, c))) for j in range(c)])


def spec_of(kind, c, l):
    return {"or": or_table, "equal": equal_table, "less_than": less_than_table}[kind](c, l)


def table_of(hl, kind, c, l):
    if kind == "or":
        return hl.LassoTable.bitwise(hl.SUBTABLE_OR, c, l)
    return hl.LassoTable.equal(c, l) if kind == "equal" else hl.LassoTable.less_than(c, l)


def operands(dims, l):
    """the two (c l/2)-bit operands of every lookup, recombined from the chunk columns (chunk 0 least significant)"""
    h = l // 2
    xs = [sum((d[k] >> h) << (h * j) for j, d in enumerate(dims)) for k in range(len(dims[0]))]
    ys = [sum((d[k] & ((1 << h) - 1)) << (h * j) for j, d in enumerate(dims)) for k in range(len(dims[0]))]
    return xs, ys


def random_dims(kind, c, l, n):
    """the chunk columns of the GPU tests' random cases (and of tests/golden/make_brakedown_lasso_tables.py): seeded by the case,
    equal operands in a third of the lookups - random ones are rarely equal"""
    import random
    import zlib
    rng = random.Random(zlib.crc32(repr((kind, c, l, n)).encode()))
    dims = [[rng.randrange(1 << l) for _ in range(1 << n)] for _ in range(c)]
    for k in range(0, 1 << n, 3):
        for j in range(c):
            dims[j][k] = (dims[j][k] >> (l // 2)) * ((1 << (l // 2)) + 1)
    return dims
