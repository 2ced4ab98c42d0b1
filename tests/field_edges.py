"""Edge tables and a big-integer reference for the field and curve primitives (csrc/ff.cuh, wide.cuh, ec.cuh), run
through the test-only probe library halo2-lasso_amd/libff_probe.so (csrc/ff_probe.hip).

Every value handed to the probe is a STORED value: the 8 little-endian u32 limbs of the Montgomery form (value * R mod
p, R = 2^256).  The reference works on stored integers: a Montgomery product of stored a, b is a b R^-1 mod p, and the
unreduced result of the product-scanning forms is exactly T = (S + ((-S p^-1) mod R) p) / R for S the sum of the
operand products.  The tables are chosen from T, so that every conditional subtraction of the kernels is seen both taken
and not taken; `band_counts` lets the tests assert that coverage instead of trusting it.

check_field_op, check_dot, check_wide and check_curve return a list of failure lines (empty: all cases passed), each
naming the op, K, field and case.  Their `run` is Probe(...).runner(host): the probe's device or host entry.
"""
import ctypes as C
import functools
import os
import random
import zlib
from array import array

from oracle.pyref import curve
from oracle.pyref.field import Q_MOD, R_MOD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(ROOT, "halo2-lasso_amd", "libff_probe.so")

OPS = ["add", "sub", "neg", "dbl", "mul", "mul_scan", "sqr", "dot_scan", "dot_cols", "mul_lazy", "add_lazy", "sub_lazy",
       "canon", "is_zero_lazy", "to_mont", "from_mont", "from_u64", "inv", "pow", "wide", "ec_dbl_affine", "ec_dbl",
       "ec_add_mixed", "ec_add_mixed_lazy", "ec_add", "ec_dbl_quad", "ec_add_quad"]
OP_ID = {name: i for i, name in enumerate(OPS)}
FIELDS = {"Fr": (0, R_MOD), "Fq": (1, Q_MOD)}
R = 1 << 256
M32 = (1 << 32) - 1
MAX_CASES = 1 << 16
DOT_KS = [1, 2, 3, 4, 5, 6, 7, 8, 10, 11, 15, 16]
FIELD_OPS = ["add", "sub", "neg", "dbl", "mul", "mul_scan", "sqr", "mul_lazy", "add_lazy", "sub_lazy", "canon",
             "is_zero_lazy", "to_mont", "from_mont", "from_u64", "inv", "pow"]
CURVE_OPS = ["ec_dbl_affine", "ec_dbl", "ec_add_mixed", "ec_add_mixed_lazy", "ec_add", "ec_dbl_quad", "ec_add_quad"]
DEVICE_ONLY = {"wide", "ec_add_mixed_lazy", "ec_dbl_quad", "ec_add_quad"}  # no host form in the headers


def nred(k):
    """the conditional subtractions ff.cuh's dot_scan / dot_scan_cols apply for K products"""
    return 1 if k <= 5 else 2 if k <= 10 else 3 if k <= 15 else 4


def limbs(x, n=8):
    return [(x >> (32 * i)) & M32 for i in range(n)]


def from_limbs(ws):
    return sum(w << (32 * i) for i, w in enumerate(ws))


@functools.lru_cache(maxsize=None)
def _neg_pinv(p):
    return (-pow(p, -1, R)) % R


def mont_t(s, p):
    """the unreduced Montgomery result of the operand-product sum s: (s + m p) / R, m = -s p^-1 mod R"""
    m = s * _neg_pinv(p) % R
    return (s + m * p) >> 256


def band_of(s, p):
    return mont_t(s, p) // p


# ------------------------------------------------------------------ the probe
class Probe:
    def __init__(self):
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("%s is missing: build it with `make -C halo2-lasso_amd/csrc`" % LIB_PATH)
        self.lib = C.CDLL(LIB_PATH)
        for name in ("ffp_run", "ffp_run_host"):
            fn = getattr(self.lib, name)
            fn.restype = C.c_int
            fn.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int]

    def runner(self, host):
        fn = self.lib.ffp_run_host if host else self.lib.ffp_run

        def run(op, field, k, cases, in_stride, out_stride):
            """cases: lists of u32 words (each at most in_stride long); returns one list of out_stride words per case"""
            n = len(cases)
            assert 0 < n <= MAX_CASES, (op, n)
            inp = array("I", bytes(4 * n * in_stride))
            for i, c in enumerate(cases):
                inp[i * in_stride:i * in_stride + len(c)] = array("I", c)
            out = array("I", bytes(4 * n * out_stride))
            ia, oa = inp.buffer_info()[0], out.buffer_info()[0]
            st = fn(OP_ID[op], FIELDS[field][0], k, ia, in_stride, oa, out_stride, n)
            assert st == 0, "%s K=%d %s: the probe returned status %d for %d cases" % (op, k, field, st, n)
            return [list(out[i * out_stride:(i + 1) * out_stride]) for i in range(n)]

        return run


# ------------------------------------------------------------------ edge tables (stored values)
@functools.lru_cache(maxsize=None)
def stored_edges(p):
    """canonical stored values (< p) at the limb and carry edges"""
    top = p >> 224
    v = [
        ((top - 1) << 224) | ((1 << 224) - 1),  # all 0xffffffff below a top limb under p's
        from_limbs([M32, 0] * 4), from_limbs([0, M32] * 3 + [0, top - 1]),  # alternating zero and all-ones limbs
        from_limbs([0, M32] * 4) % p, from_limbs([M32, 0] * 3 + [M32, top - 1]),
        p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, R % p, (R * R) % p, 1, 2, 0,  # 1: the stored value of R^-1
        (p - 1) & ~M32, (R % p) & ~M32, p & ~M32,  # low limb 0: first Montgomery digit 0 against any operand
        p & M32, (p - 1) >> 32 << 32 | (p & M32) - 2,  # low limb near p's
    ]
    for kbit in list(range(0, 256, 32)) + [253]:
        v += [(1 << kbit) - 1, 1 << kbit, (1 << kbit) + 1]
    out = []
    for x in v:
        x %= p
        if x not in out:
            out.append(x)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def lazy_edges(p):
    """stored values in [0, 2 p): the canonical edges, p, p + 1, 2 p - 1 and x + p for every canonical edge x"""
    out = list(stored_edges(p)) + [p, p + 1, 2 * p - 1, 2 * p - 2]
    out += [x + p for x in stored_edges(p) if x + p not in out]
    return tuple(out)


def _rand(rng, p, n):
    return [rng.randrange(p) for _ in range(n)]


def m_digit_pairs(p, rng, n=24):
    """pairs whose first Montgomery digit m = a0 b0 (-p^-1) mod 2^32 is 2^32 - 1 (a0 b0 = p0 mod 2^32), and pairs with
    m = 0 (a0 b0 = 0 mod 2^32)"""
    p0 = p & M32
    out = []
    for i in range(n):
        b = rng.randrange(p) | 1 if i else 1
        a0 = p0 * pow(b & M32, -1, 1 << 32) % (1 << 32)
        a = ((rng.randrange(p) >> 32 << 32) | a0) % p if i else p0
        if (a & M32) * (b & M32) % (1 << 32) == p0:
            out.append((a, b))
        a = rng.randrange(p) >> 32 << 32
        out.append((a, rng.randrange(p)))
    return out


def band_pairs(p, rng, lo_band, hi_band, per_band=6):
    """canonical pairs whose unreduced product lands in each band [j p, (j + 1) p), j = lo_band .. hi_band"""
    got = {j: [] for j in range(lo_band, hi_band + 1)}
    for _ in range(200000):
        if all(len(v) >= per_band for v in got.values()):
            break
        a, b = p - 1 - rng.randrange(1 << rng.choice((8, 64, 200, 250))), rng.randrange(p)
        j = band_of(a * b, p)
        if j in got and len(got[j]) < per_band:
            got[j].append((a, b))
    assert all(len(v) >= per_band for v in got.values()), {j: len(v) for j, v in got.items()}
    return [x for v in got.values() for x in v]


def dot_cases(p, k, rng):
    """operand vectors (a[0..k), b[0..k)) for dot<k>: every band [j p, (j + 1) p) of the unreduced result up to
    nred(k), the top band included, found by search around near-maximal operands; plus the edge tables"""
    top = nred(k)
    got = {j: [] for j in range(top + 1)}
    s_max = k * (p - 1) ** 2 / (R * p)  # the largest operand sum, in units of R p
    for j in range(top + 1):
        target = min(max(j - 0.5, 0.0), s_max)
        b_base = int(target * R * p / (k * (p - 1)))
        for _ in range(100000):
            if len(got[j]) >= 6:
                break
            a = [p - 1 - rng.randrange(1 << 32) for _ in range(k)]
            b = [min(p - 1, max(0, b_base - rng.randrange(1 << 230))) for _ in range(k)]
            if band_of(sum(x * y for x, y in zip(a, b)), p) == j:
                got[j].append((a, b))
        assert len(got[j]) >= 6, "dot<%d>: band %d not reached" % (k, j)
    cases = [c for j in range(top + 1) for c in got[j]]
    e = stored_edges(p)
    for i, x in enumerate(e):
        cases.append(([x] * k, [e[(i * 7 + 3) % len(e)]] * k))
        cases.append(([x] * k, [x] * k))
    cases.append(([p - 1] * k, [p - 1] * k))
    cases.append(([0] * k, [p - 1] * k))
    for _ in range(64):
        cases.append((_rand(rng, p, k), _rand(rng, p, k)))
        cases.append(([rng.choice(e) for _ in range(k)], [rng.choice(e) for _ in range(k)]))
    return cases


def band_counts(p, cases):
    out = {}
    for a, b in cases:
        j = band_of(sum(x * y for x, y in zip(a, b)), p)
        out[j] = out.get(j, 0) + 1
    return out


# ------------------------------------------------------------------ field ops: inputs and reference
def field_cases(op, p, seed=0):
    """(inputs, expected, kind): kind 'canon' (exact, < p), 'lazy' (= mod p, < 2 p) or 'bool'"""
    rng = random.Random(zlib.crc32(("%s %x %d" % (op, p, seed)).encode()))
    e, lz = list(stored_edges(p)), list(lazy_edges(p))
    canon_pairs = [(a, b) for a in e for b in e] + [(a, b) for a, b in zip(_rand(rng, p, 256), _rand(rng, p, 256))]
    lazy_pairs = [(a, b) for a in lz for b in lz] + [(rng.randrange(2 * p), rng.randrange(2 * p)) for _ in range(256)]
    ri = pow(R, -1, p)
    unary = e + _rand(rng, p, 64)
    if op in ("add", "sub"):
        f = (lambda a, b: (a + b) % p) if op == "add" else (lambda a, b: (a - b) % p)
        return [[a, b] for a, b in canon_pairs], [f(a, b) for a, b in canon_pairs], "canon"
    if op in ("mul", "mul_scan"):
        pairs = canon_pairs + m_digit_pairs(p, rng) + band_pairs(p, rng, 0, 1)
        return [[a, b] for a, b in pairs], [a * b * ri % p for a, b in pairs], "canon"
    if op == "sqr":
        xs = unary + [a for a, _ in band_pairs(p, rng, 0, 1)]
        return [[x] for x in xs], [x * x * ri % p for x in xs], "canon"
    if op in ("neg", "dbl"):
        return [[x] for x in unary], [(-x if op == "neg" else 2 * x) % p for x in unary], "canon"
    if op == "mul_lazy":
        return [[a, b] for a, b in lazy_pairs], [a * b * ri % p for a, b in lazy_pairs], "lazy"
    if op in ("add_lazy", "sub_lazy"):
        f = (lambda a, b: (a + b) % p) if op == "add_lazy" else (lambda a, b: (a - b) % p)
        return [[a, b] for a, b in lazy_pairs], [f(a, b) for a, b in lazy_pairs], "lazy"
    if op == "canon":
        xs = lz + [rng.randrange(2 * p) for _ in range(64)]
        return [[x] for x in xs], [x % p for x in xs], "canon"
    if op == "is_zero_lazy":
        xs = lz + [rng.randrange(2 * p) for _ in range(64)]
        return [[x] for x in xs], [int(x % p == 0) for x in xs], "bool"
    if op in ("to_mont", "from_mont"):  # any 256-bit integer: the product stays below 2 p
        xs = unary + [R - 1, R >> 1, p, 2 * p - 1, 2 * p, R - p, (R - 1) & ~M32]
        f = (lambda x: x * R % p) if op == "to_mont" else (lambda x: x * ri % p)
        return [[x] for x in xs], [f(x) for x in xs], "canon"
    if op == "from_u64":
        xs = [0, 1, 2, M32, 1 << 32, (1 << 64) - 1, (1 << 63), (1 << 63) - 1] + [rng.randrange(1 << 64) for _ in range(64)]
        return [[x] for x in xs], [x * R % p for x in xs], "canon"
    if op == "inv":  # stored a = x R -> x^-1 R = R^2 a^-1; zero maps to zero
        return [[x] for x in unary], [(R * R * pow(x, -1, p)) % p if x else 0 for x in unary], "canon"
    if op == "pow":
        exps = [0, 1, 2, 3, p - 1, p - 2, (p - 1) // 2, R - 1, M32, 1 << 32, 1 << 253] + _rand(rng, p, 4)
        bases = [0, 1, R % p, p - 1, (p + 1) // 2, e[0]] + _rand(rng, p, 2)
        cases = [(a, x) for a in bases for x in exps]
        return [[a, x] for a, x in cases], [pow(a * ri, x, p) * R % p for a, x in cases], "canon"
    raise KeyError(op)


def dot_lazy_cases(p, rng):
    """dot<2> on LAZY operands, as add_mixed_lazy uses it: the result must be below 2 p after its one subtraction"""
    lz = list(lazy_edges(p))
    cases = [([lz[i], lz[j]], [lz[j], lz[i]]) for i in range(0, len(lz), 3) for j in range(len(lz))]
    cases += [([2 * p - 1 - rng.randrange(1 << 32) for _ in range(2)], [2 * p - 1 - rng.randrange(1 << 32) for _ in range(2)])
              for _ in range(256)]
    return cases


def _check_values(op, field, k, p, cases, outs, expected, kind, describe):
    bad = []
    for i, (o, want) in enumerate(zip(outs, expected)):
        if kind == "bool":
            got = o[0]
            ok = got == want
        else:
            got = from_limbs(o[:8])
            ok = got == want if kind == "canon" else (got < 2 * p and got % p == want % p)
        if not ok:
            bad.append("%s K=%d %s case %d (%s): got 0x%x, want %s0x%x" % (
                op, k, field, i, describe(cases[i]), got, "" if kind != "lazy" else "< 2p and = mod p ", want))
    return bad


def check_field_op(run, op, field):
    p = FIELDS[field][1]
    ins, expected, kind = field_cases(op, p)
    if op == "from_u64":
        cases = [[x & M32, x >> 32] for (x,) in ins]
    else:
        cases = [sum((limbs(x) for x in c), []) for c in ins]
    outs = run(op, field, 0, cases, max(len(c) for c in cases), 8)
    return _check_values(op, field, 0, p, ins, outs, expected, kind, lambda c: ", ".join("0x%x" % x for x in c))


def check_dot(run, form, field, k, lazy=False):
    p = FIELDS[field][1]
    rng = random.Random(1000 * k + FIELDS[field][0] + 7 * lazy)
    cases = dot_lazy_cases(p, rng) if lazy else dot_cases(p, k, rng)
    if not lazy and sorted(band_counts(p, cases)) != list(range(nred(k) + 1)):
        return ["%s K=%d %s: the table misses a band: %s" % (form, k, field, band_counts(p, cases))]
    ri = pow(R, -1, p)
    expected = [sum(x * y for x, y in zip(a, b)) * ri % p for a, b in cases]
    words = [sum((limbs(x) for x in a + b), []) for a, b in cases]
    outs = run(form, field, k, words, 16 * k, 8)
    return _check_values(form + ("[lazy operands]" if lazy else ""), field, k, p, cases, outs, expected,
                         "lazy" if lazy else "canon",
                         lambda c: "band %d, a=[%s] b=[%s]" % (band_of(sum(x * y for x, y in zip(*c)), p),
                                                               ", ".join("0x%x" % x for x in c[0]),
                                                               ", ".join("0x%x" % x for x in c[1])))


# ------------------------------------------------------------------ Wide (Fr)
def wide_cases(seed=0):
    """(start, [(w, v)]): the accumulator start value and the wide_mac terms; every final sum is below 2^320"""
    r = R_MOD
    rng = random.Random(seed)
    big = (r - 1, M32)
    term = (r - 1) * M32
    cases = [(0, []), (0, [(0, M32)] * 3), (0, [(r - 1, 0)] * 3)]  # a zero accumulator
    cases += [(0, [big] * t) for t in (1, 2, 3, 16, 64)]
    for bound in (1 << 256, 1 << 288):  # carries into limb 8, limb 9, and across the boundary
        for tm in ((r - 1, 1), (r - 1, 5), big):
            for d in (-2, -1, 0, 1, 1 << 32):
                if 2 * tm[0] * tm[1] < bound:
                    cases.append((bound - tm[0] * tm[1] + d, [tm]))
                    cases.append((bound - 2 * tm[0] * tm[1] + d, [tm, tm]))
    for d in (-1, -2, -(1 << 32), -(1 << 64)):  # up to the documented bound 2^320
        cases.append(((1 << 320) + d - term, [big]))
        cases.append(((1 << 320) + d - 3 * term, [big] * 3))
    cases.append(((1 << 320) - 1, []))
    # wide_redc's unreduced result (acc + m r) / R is r + t exactly when acc = k r + t R (then m = R - k): the final
    # conditional subtraction is needed; t up to 2^64 - 1 keeps acc below 2^320
    for kk, t in ((1, 0), (1, 1), (2, 0), (3, 1 << 32), (1, (1 << 64) - 1), (5, (1 << 63) + 12345)):
        cases.append((kk * r + t * R, []))
    for _ in range(24):
        kk, t = rng.randrange(1, 1 << 40), rng.randrange(1 << 63)
        acc = kk * r + t * R
        cases.append((acc - term, [big]) if acc >= term else (acc, []))
    # hi = 0 (the sum stays below 2^256) and hi != 0 with small-valued columns, as Lasso feeds them
    e = [x for x in stored_edges(r)]
    cases.append((0, [(w, (i * 2654435761) & 0xffff) for i, w in enumerate(e[:32])]))
    cases.append((0, [(w, M32 - i) for i, w in enumerate(e[:32])]))
    cases.append(((1 << 256) - 1, [(1, 1)]))
    cases.append(((1 << 256) - 2, [(1, 1)]))
    # weights pre-scaled as prescale_r does (stored x R^2): wide_redc then returns the stored form of sum x v
    xs = _rand(rng, r, 8) + [r - 1, 1, 0]
    cases.append((0, [(x * R * R % r, rng.randrange(1 << 16)) for x in xs]))
    cases.append((0, [(x * R * R % r, M32) for x in xs]))
    for _ in range(32):
        terms = [(rng.randrange(r), rng.randrange(1 << 32)) for _ in range(rng.randrange(1, 12))]
        cases.append((rng.randrange(1 << rng.choice((0, 200, 256, 290, 300))), terms))
    for s, terms in cases:
        assert 0 <= s and s + sum(w * v for w, v in terms) < 1 << 320, (hex(s), len(terms))
    return cases


def check_wide(run):
    r = R_MOD
    ri = pow(R, -1, r)
    cases = wide_cases()
    stride = 11 + 9 * max(len(t) for _, t in cases)
    words = [limbs(s, 10) + [len(t)] + sum((limbs(w) + [v] for w, v in t), []) for s, t in cases]
    outs = run("wide", "Fr", 0, words, stride, 26)
    bad = []
    for i, ((s, terms), o) in enumerate(zip(cases, outs)):
        acc = s + sum(w * v for w, v in terms)
        raw, red, redc = from_limbs(o[:10]), from_limbs(o[10:18]), from_limbs(o[18:26])
        what = "wide case %d (start 0x%x, %d terms, sum 0x%x)" % (i, s, len(terms), acc)
        if raw != acc:
            bad.append("%s: raw limbs 0x%x" % (what, raw))
        if red != acc % r:
            bad.append("%s: wide_reduce 0x%x, want 0x%x" % (what, red, acc % r))
        if redc != acc * ri % r:
            bad.append("%s: wide_redc 0x%x, want 0x%x" % (what, redc, acc * ri % r))
    return bad


# ------------------------------------------------------------------ curves (Fq)
def _mont(x):
    return x * R % Q_MOD


def _unmont(x):
    return x * pow(R, -1, Q_MOD) % Q_MOD


@functools.lru_cache(maxsize=None)
def curve_tables():
    """affine points (identity, G, 2G, a random point, their negatives) and XYZZ forms (l^2 x, l^3 y, l^2, l^3)"""
    rng = random.Random(11)
    g = curve.G1_GEN
    g2 = curve.add(g, g)
    rp = curve.mul(g, rng.randrange(1, R_MOD))
    aff = [None, g, g2, rp, curve.neg(g), curve.neg(rp)]
    lams = [1, 2, Q_MOD - 1, rng.randrange(2, Q_MOD)]
    xyzz = [(None, None)]
    for pt in aff[1:]:
        for lam in lams:
            x, y = pt
            vals = (lam * lam * x % Q_MOD, lam ** 3 * y % Q_MOD, lam * lam % Q_MOD, lam ** 3 % Q_MOD)
            xyzz.append((pt, tuple(_mont(v) for v in vals)))
    return aff, xyzz


def _aff_words(pt):
    return [0] * 16 if pt is None else limbs(_mont(pt[0])) + limbs(_mont(pt[1]))


def _xyzz_words(stored):
    return [0] * 32 if stored is None else sum((limbs(c) for c in stored), [])


def _check_xyzz(o, want, bound):
    """None, or what is wrong with the stored XYZZ limbs o against the affine point want"""
    c = [from_limbs(o[8 * i:8 * i + 8]) for i in range(4)]
    if any(v >= bound for v in c):
        return "coordinate above %s" % ("q" if bound == Q_MOD else "2q")
    x, y, zz, zzz = (_unmont(v) for v in c)
    if zz == 0:
        if c[2] != 0:
            return "ZZ = q, not 0"
        return None if want is None else "identity, want (0x%x, 0x%x)" % want
    if zz ** 3 % Q_MOD != zzz ** 2 % Q_MOD:
        return "ZZ^3 != ZZZ^2"
    got = (x * pow(zz, -1, Q_MOD) % Q_MOD, y * pow(zzz, -1, Q_MOD) % Q_MOD)
    if want is None or got != want:
        return "affine (0x%x, 0x%x), want %s" % (got + ("identity" if want is None else "(0x%x, 0x%x)" % want,))
    return None


def curve_cases(op):
    """(words, [(out offset, expected affine point, coordinate bound)], description) per case"""
    aff, xyzz = curve_tables()
    out = []
    if op == "ec_dbl_affine":
        for pt in aff:
            out.append((_aff_words(pt), [(0, curve.add(pt, pt), Q_MOD)], "P=%s" % (pt,)))
    elif op in ("ec_dbl", "ec_dbl_quad"):
        for pt, st in xyzz:
            want = curve.add(pt, pt)
            lanes = 4 if op == "ec_dbl_quad" else 1
            out.append((_xyzz_words(st), [(32 * l, want, Q_MOD) for l in range(lanes)], "P=%s xyzz=%s" % (pt, st)))
    elif op in ("ec_add", "ec_add_quad"):
        lanes = 4 if op == "ec_add_quad" else 1
        for pt, st in xyzz:
            for qt, sq in xyzz:
                out.append((_xyzz_words(st) + _xyzz_words(sq), [(32 * l, curve.add(pt, qt), Q_MOD) for l in range(lanes)],
                            "P=%s xyzz=%s Q=%s xyzz=%s" % (pt, st, qt, sq)))
    elif op in ("ec_add_mixed", "ec_add_mixed_lazy"):
        accs = [(pt, st, "") for pt, st in xyzz]
        if op == "ec_add_mixed_lazy":  # lazy accumulators: coordinates replaced by coordinate + q
            for pt, st in xyzz[1:]:
                for mask in (0b1111, 0b0001, 0b0010, 0b0100, 0b1000, 0b0011):
                    accs.append((pt, tuple(c + Q_MOD * ((mask >> i) & 1) for i, c in enumerate(st)), " +q mask %d" % mask))
        for pt, st, tag in accs:
            for qt in aff:
                for negate in (0, 1):
                    want = curve.add(pt, curve.neg(qt) if negate else qt)
                    checks = [(0, want, Q_MOD)] if op == "ec_add_mixed" else [(0, want, 2 * Q_MOD), (32, want, Q_MOD)]
                    out.append((_xyzz_words(st) + _aff_words(qt) + [negate], checks,
                                "P=%s xyzz=%s%s Q=%s negate=%d" % (pt, st, tag, qt, negate)))
    else:
        raise KeyError(op)
    return out


def check_curve(run, op):
    cases = curve_cases(op)
    out_words = {"ec_add_mixed_lazy": 64, "ec_dbl_quad": 128, "ec_add_quad": 128}.get(op, 32)
    outs = run(op, "Fq", 0, [w for w, _, _ in cases], max(len(w) for w, _, _ in cases), out_words)
    bad = []
    for i, ((_, checks, what), o) in enumerate(zip(cases, outs)):
        for off, want, bound in checks:
            err = _check_xyzz(o[off:off + 32], want, bound)
            if err:
                bad.append("%s Fq case %d (%s), output word %d: %s" % (op, i, what, off, err))
        if op in ("ec_dbl_quad", "ec_add_quad") and any(o[32 * l:32 * l + 32] != o[:32] for l in range(1, 4)):
            bad.append("%s Fq case %d (%s): the four quad lanes disagree" % (op, i, what))
    return bad


def report(bad, limit=12):
    return "%d failures:\n%s" % (len(bad), "\n".join(bad[:limit]))
