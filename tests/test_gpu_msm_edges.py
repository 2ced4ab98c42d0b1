"""MSM and KZG commitments on degenerate bases and digit-edge scalars, at every default route of csrc/msm.hip.

With random distinct bases two partial sums of an MSM are equal or opposite with probability ~2^-254, so the "same x"
branches of every stage past the first (continuation levels, segment and group reductions, window sums: `add`,
`add_quad` / `dbl_quad`, `mul_small` / `mul_small_quad`) never run in the parity tests, and uniformly random scalars
never hit the signed-digit boundaries of window widths 5..17.  Here every base is a KNOWN multiple e_i G of the
generator, so the MSM has a closed form independent of the device and of the C++ oracle's Pippenger:
    sum_i s_i (e_i G) = (sum_i s_i e_i mod r) G
(`Multiples.expected`: s_i is read back from the Montgomery bytes that were uploaded).  A trapdoor with equal
coordinates makes the multilinear KZG SRS such a table as well: level k holds eq(b; s) G = s^|b| (1 - s)^(k - |b|) G
(|b| = popcount), so commit(poly) = poly~(s) G - s = 1/2 gives 2^-k G at every point of a level, s = 2 and s = -1 give
only +-2^j G.  Proofs over such an SRS must still be the C++ oracle's bytes and verify.

Sizes: n = 2^8, 2^12, 2^16, 2^20 - 3 run at window widths c = 4, 8, 12, 15, with 4-, 8-bucket segments, slab sorts from
2^16 on; `all_equal` scalars on equal bases at 2^20 - 3 make one hot bucket of ~2^20 entries per window whose
continuation list (~2^19 chunk sums, all equal) goes through linear (plain) levels and then tree levels.  The other
shapes - c = 5, 7, 11, 13, 17, plain (not quad-cooperative) kernels, the two-level group reduction, 16-bucket segments,
fan-in 2, pipelined half batches - are forced in child processes by test_small_edges_under_forced_msm_shapes, which
reruns the MSM and commit cases whose ids carry `small`.
"""
import os
import random

import numpy as np
import pytest

from oracle.pyref import curve
from oracle.pyref.field import MONT_R, Q_MOD, R_MOD as P

G = curve.G1_GEN
_MONT = MONT_R % P
_MONT_INV = pow(_MONT, -1, P)
TOP_LIMB = 0x30644E72E131A029  # top 64 bits of r


# ------------------------------------------------------------------ reference helper (no GPU)
def g1_enc(pt):
    """affine point (or None) -> the 64 Montgomery bytes of a bn256::G1Affine"""
    if pt is None:
        return bytes(64)
    return b"".join((v * MONT_R % Q_MOD).to_bytes(32, "little") for v in pt)


def mont_rows(values):
    """canonical field elements -> (len, 4) uint64 rows of their Montgomery limbs"""
    raw = b"".join((v % P * _MONT % P).to_bytes(32, "little") for v in values)
    return np.frombuffer(raw, dtype=np.uint64).reshape(-1, 4)


def raw_rows(limbs):
    """Montgomery limb patterns given as they are stored (each a 4-tuple, little-endian u64, value < r)"""
    return np.array(limbs, dtype=np.uint64).reshape(-1, 4)


class Multiples:
    """A table of known multiples k_t G (k_t = 0 is the identity) and their encodings.  Bases are rows of the table
    picked by an index array; the MSM over them has the closed form (sum_i s_i k_{idx_i} mod r) G."""

    def __init__(self, ks):
        self.ks = [k % P for k in ks]
        self.pts = [curve.mul(G, k) for k in self.ks]
        self.enc = np.frombuffer(b"".join(g1_enc(p) for p in self.pts), dtype=np.uint8).reshape(-1, 64)

    def bases(self, idx):
        return self.enc[np.asarray(idx)].tobytes()

    def points(self, idx):
        return [self.pts[int(i)] for i in idx]

    def _weighted(self, idx, parts, width):
        """sum_t k_t sum_{i: idx_i = t} v_i, v_i given as little-endian `width`-bit parts (float64 sums stay exact:
        every part is < 2^32 and n < 2^21)"""
        idx = np.asarray(idx)
        acc = [0] * len(self.ks)
        for j in range(parts.shape[1]):
            sums = np.bincount(idx, weights=parts[:, j], minlength=len(self.ks))
            for t, v in enumerate(sums):
                if v:
                    acc[t] += int(v) << (width * j)
        return sum(k * a for k, a in zip(self.ks, acc))

    def expected(self, scalars, idx):
        """MSM of Montgomery Fr scalars (bytes, 32 per element) over bases `idx`: from_mont is linear mod r, so the
        Montgomery values are summed per table entry first"""
        parts = np.frombuffer(scalars, dtype=np.uint16).reshape(-1, 16)
        assert parts.shape[0] == len(idx)
        return curve.mul(G, self._weighted(idx, parts, 16) * _MONT_INV % P)

    def expected_u32(self, scalars, idx):
        v = np.frombuffer(scalars, dtype=np.uint32).reshape(-1, 1)
        assert v.shape[0] == len(idx)
        return curve.mul(G, self._weighted(idx, v, 32) % P)


# the table: O, +-G, +-2G, 3G, a random P and 2P, six random multiples, +-2^j G for j < 32
T_O, T_G, T_NG, T_2G, T_N2G, T_3G, T_K, T_2K = range(8)
T_RAND = list(range(8, 14))
T_POW2 = list(range(14, 78))
ALL_T = list(range(78))


def table_multiples(seed=2024):
    rng = random.Random(seed)
    k = rng.randrange(1, P)
    ks = [0, 1, P - 1, 2, P - 2, 3, k, 2 * k] + [rng.randrange(1, P) for _ in T_RAND]
    for j in range(32):
        ks += [1 << j, P - (1 << j)]
    return Multiples(ks)


def window_bits(n, bits):
    """csrc/msm.hip pick_window: floor(log2 n) - LH_MSM_C_OFF, clamped to 4 .. LH_MSM_C_MAX, at most `bits`"""
    off = int(os.environ.get("LH_MSM_C_OFF") or 4)
    cmax = int(os.environ.get("LH_MSM_C_MAX") or 17)
    c = n.bit_length() - 1 - off
    c = max(c, 4)
    c = min(c, cmax)
    return min(c, bits)


def base_family(name, n, rng):
    i = np.arange(n)
    if name == "G":
        return np.full(n, T_G)
    if name == "pm":  # G, -G alternating: under equal scalars every pair, chunk and segment sums to O
        return np.where(i & 1, T_NG, T_G)
    if name == "id_runs":  # runs of 2^k identity bases between runs of table points
        k = (n.bit_length() - 1) // 2
        return np.where((i >> k) & 1, rng.choice(ALL_T, size=n), T_O)
    if name == "id_every_other":
        return np.where(i & 1, rng.choice(ALL_T, size=n), T_O)
    if name == "p_2p":  # P interleaved with 2P
        return np.where(i & 1, T_2K, T_K)
    if name == "pow2":  # +-2^j G only: the points of a trapdoor-2 SRS
        return rng.choice(T_POW2, size=n)
    if name == "table":
        return rng.choice(ALL_T, size=n)
    raise ValueError(name)


BASE_FAMILIES = ["G", "pm", "id_runs", "id_every_other", "p_2p", "pow2", "table"]


def fr_family(name, n, rng):
    """-> Montgomery bytes of n scalars; `c` is the window width the MSM will use for them"""
    c = window_bits(n, 254)
    pick = lambda rows: np.ascontiguousarray(rows[rng.integers(0, len(rows), size=n)])
    cycle = lambda rows: np.ascontiguousarray(rows[np.arange(n) % len(rows)])
    x = int(rng.integers(1, 1 << 62)) * int(rng.integers(1, 1 << 62)) * int(rng.integers(1, 1 << 62)) % P
    if name == "one_nonzero":
        a = np.zeros((n, 4), dtype=np.uint64)
        a[int(rng.integers(0, n))] = mont_rows([x])[0]
        return a.tobytes()
    if name == "all_equal":
        return np.repeat(mont_rows([x]), n, axis=0).tobytes()
    if name == "r_minus_1":
        return np.repeat(mont_rows([P - 1]), n, axis=0).tobytes()
    if name == "ones_253":  # every window's digit 2^c - 1 is -1 with a carry: the carries run into the head-room window
        return np.repeat(mont_rows([(1 << 253) - 1]), n, axis=0).tobytes()
    if name == "half_digits":  # every digit exactly +2^(c-1): the largest positive signed digit, no carry
        v = sum(1 << (c * w + c - 1) for w in range(254) if c * w + c - 1 <= 252)
        return np.repeat(mont_rows([v]), n, axis=0).tobytes()
    if name == "window_edges":  # 2^(cw) - 1 (a carry through w windows) and 2^(cw) (one digit 1 in window w)
        vals = [0]
        for w in range(1, 254):
            if c * w > 253:
                break
            vals += [(1 << (c * w)) - 1, 1 << (c * w)]
        return cycle(mont_rows(vals)).tobytes()
    if name == "mont_limbs":  # extreme STORED limbs (the values themselves look random)
        return cycle(MONT_EXTREMES).tobytes()
    if name == "mixed":
        vals = [0, 1, 2, P - 1, P - 2, (1 << 253) - 1, (P - 1) // 2, x]
        vals += [(1 << (c * w)) - 1 for w in range(1, 254) if c * w <= 253]
        vals += [1 << (c * w + c - 1) for w in range(0, 254) if c * w + c - 1 <= 252]
        return pick(np.concatenate([mont_rows(vals), MONT_EXTREMES])).tobytes()
    raise ValueError(name)


M64 = (1 << 64) - 1
MONT_EXTREMES = raw_rows([
    [((P - 1) >> (64 * j)) & M64 for j in range(4)],                # stored limbs r - 1
    [M64, M64, M64, TOP_LIMB - 1],                                   # all-ones limbs under the top one
    [0xffffffff] * 3 + [0xffffffff],                                 # 32-bit halves of ones / zeros
    [0xffffffff00000000] * 3 + [0xffffffff],
    [1, 0, 0, 0],                                                    # stored 1 (the value R^-1)
    [0, 0, 0, 1 << 32],
    [M64, 0, M64, 0x30000000ffffffff],
])
FR_FAMILIES = ["one_nonzero", "all_equal", "r_minus_1", "ones_253", "half_digits", "window_edges", "mont_limbs", "mixed"]


def u32_family(name, n, rng):
    c = window_bits(n, 32)
    if name == "zero_one_max":
        v = rng.choice(np.array([0, 1, 0xffffffff], dtype=np.uint32), size=n)
    elif name == "c_edges":  # 2^c - 1 and 2^c: all ones in window 0, a single one in window 1
        v = rng.choice(np.array([0, (1 << c) - 1, 1 << c], dtype=np.uint32), size=n)
    elif name == "top_partial":  # only the bits of the (partial) top window
        top = 32 - (32 % c or c)
        v = (rng.integers(1, 1 << (32 - top), size=n, dtype=np.uint64) << top).astype(np.uint32)
        v[0] = ((1 << (32 - top)) - 1) << top
    elif name == "all_equal":
        v = np.full(n, 0x80000000 | int(rng.integers(0, 1 << 31)), dtype=np.uint32)
    elif name == "one_nonzero":
        v = np.zeros(n, dtype=np.uint32)
        v[int(rng.integers(0, n))] = 0xffffffff
    else:
        raise ValueError(name)
    return v.astype(np.uint32).tobytes()


U32_FAMILIES = ["zero_one_max", "c_edges", "top_partial", "all_equal", "one_nonzero"]


def test_reference_helper_matches_curve_msm():
    """the closed form against the Python oracle's Pippenger, on every family at small n"""
    mult = table_multiples()
    rng = np.random.default_rng(1)
    for n in (1, 2, 17, 64):
        for bf in BASE_FAMILIES:
            idx = base_family(bf, n, rng)
            pts = mult.points(idx)
            for sf in FR_FAMILIES:
                s = fr_family(sf, n, rng)
                ints = [int.from_bytes(s[32 * i:32 * i + 32], "little") * _MONT_INV % P for i in range(n)]
                assert mult.expected(s, idx) == curve.msm(ints, pts), (n, bf, sf)
            for uf in U32_FAMILIES:
                s = u32_family(uf, n, rng)
                assert mult.expected_u32(s, idx) == curve.msm(list(np.frombuffer(s, np.uint32).tolist()), pts), (n, bf, uf)


def test_degenerate_srs_levels_are_the_closed_form():
    """eq(b; s) for equal trapdoor coordinates depends on popcount(b) only: the Python oracle's setup agrees"""
    from oracle.pyref import kzg as o_kzg
    for s in TRAPDOORS.values():
        opp = o_kzg.setup([s] * 4)
        for k in range(5):
            assert opp.eqs[k] == level_multiples(s, k).points(popcount(k)), (s, k)


# ------------------------------------------------------------------ degenerate trapdoors
TRAPDOORS = {"half": (P + 1) // 2, "two": 2, "minus_one": P - 1}


def popcount(k):
    return np.bitwise_count(np.arange(1 << k, dtype=np.uint64)).astype(np.int64)


def level_multiples(s, k):
    """level k of the SRS of trapdoor (s, .., s): entry b is s^|b| (1 - s)^(k - |b|) G - a table indexed by popcount"""
    return Multiples([pow(s, j, P) * pow(1 - s, k - j, P) for j in range(k + 1)])


# ------------------------------------------------------------------ GPU
SIZES = [pytest.param(1 << 8, id="small-256"), pytest.param(1 << 12, id="small-4096"),
         pytest.param(1 << 16, id="large-65536"), pytest.param((1 << 20) - 3, id="large-1048573")]


@pytest.fixture(scope="module")
def mult():
    return table_multiples()


@pytest.fixture(scope="module")
def base_cache(mult, ctx):
    """(n, family) -> (index array, device bases): built once per module"""
    cache = {}

    def get(n, fam):
        if (n, fam) not in cache:
            idx = base_family(fam, n, np.random.default_rng(n + BASE_FAMILIES.index(fam)))
            cache[(n, fam)] = idx, ctx.upload(mult.bases(idx))
        return cache[(n, fam)]
    yield get
    for _, buf in cache.values():
        buf.free()


@pytest.mark.gpu
@pytest.mark.parametrize("family", FR_FAMILIES)
@pytest.mark.parametrize("n", SIZES)
def test_msm_fr_degenerate(hl, ctx, mult, base_cache, n, family):
    rng = np.random.default_rng(n * 31 + FR_FAMILIES.index(family))
    s = fr_family(family, n, rng)
    ds = ctx.upload(s)
    for bf in BASE_FAMILIES:
        idx, db = base_cache(n, bf)
        assert hl.variable_base_msm(ctx, ds, db, n) == mult.expected(s, idx), (family, bf, "c = %d" % window_bits(n, 254))
    ds.free()


@pytest.mark.gpu
@pytest.mark.parametrize("family", U32_FAMILIES)
@pytest.mark.parametrize("n", SIZES)
def test_msm_u32_degenerate(hl, ctx, mult, base_cache, n, family):
    rng = np.random.default_rng(n * 37 + U32_FAMILIES.index(family))
    s = u32_family(family, n, rng)
    ds = ctx.upload(s)
    for bf in BASE_FAMILIES:
        idx, db = base_cache(n, bf)
        assert hl.variable_base_msm_u32(ctx, ds, db, n) == mult.expected_u32(s, idx), (family, bf, "c = %d" % window_bits(n, 32))
    ds.free()


@pytest.mark.gpu
@pytest.mark.parametrize("lg", [pytest.param(12, id="small-4096"), pytest.param(16, id="large-65536")])
def test_msm_degenerate_mixed_with_distinct_bases(hl, ctx, lg):
    """random distinct SRS points with G, -G, identity runs and repeated neighbours spliced in; the C++ oracle decides"""
    from oracle import cpu_oracle as co
    n = 1 << lg
    rng = random.Random(lg)
    pp = hl.MultilinearKzg.setup(ctx, [rng.randrange(1, P) for _ in range(lg)])
    flat = pp.eqs_bytes()
    pp.free()
    b = np.frombuffer(flat[64 * (n - 1):64 * (2 * n - 1)], dtype=np.uint8).reshape(n, 64).copy()
    i = np.arange(n)
    b[i % 3 == 0] = np.frombuffer(g1_enc(G), dtype=np.uint8)
    b[i % 7 == 1] = np.frombuffer(g1_enc(curve.neg(G)), dtype=np.uint8)
    rep = np.nonzero(i % 5 == 2)[0]
    b[rep] = b[rep - 1]
    b[n // 4:n // 4 + n // 8] = 0
    bases = b.tobytes()
    db = ctx.upload(bases)
    nrng = np.random.default_rng(lg)
    for fam in ("mixed", "all_equal", "window_edges"):
        s = fr_family(fam, n, nrng)
        assert hl.variable_base_msm(ctx, ctx.upload(s), db, n) == co.msm(s, bases), fam
    u = u32_family("zero_one_max", n, nrng)
    src = ctx.upload(u)
    as_fr = ctx.alloc(32 * n)
    hl._check(ctx.lib.lh_fr_from_u32(ctx.h, src.ptr, n, as_fr.ptr))
    ctx.sync()
    assert hl.variable_base_msm_u32(ctx, src, db, n) == co.msm(as_fr.read(), bases)


# ------------------------------------------------------------------ multilinear KZG over degenerate trapdoors
@pytest.fixture(scope="module")
def srs_cache(hl, ctx):
    """(trapdoor name, num_vars) -> (ss, device params, C++ oracle's flat SRS)"""
    from oracle import cpu_oracle as co
    cache = {}

    def get(name, nv):
        if (name, nv) not in cache:
            ss = [TRAPDOORS[name]] * nv
            cache[(name, nv)] = ss, hl.MultilinearKzg.setup(ctx, ss), co.setup(ss)
        return cache[(name, nv)]
    yield get
    for _, pp, _ in cache.values():
        pp.free()


def _level(flat, k):
    return flat[64 * ((1 << k) - 1):64 * ((2 << k) - 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TRAPDOORS))
@pytest.mark.parametrize("nv", [pytest.param(12, id="small-12"), pytest.param(17, id="large-17")])
def test_setup_degenerate_trapdoor(srs_cache, name, nv):
    ss, pp, flat = srs_cache(name, nv)
    assert pp.num_vars == nv
    assert pp.eqs_bytes() == flat, "device setup differs from the C++ oracle's"
    for k in (0, 1, 5, nv):
        assert _level(flat, k) == level_multiples(ss[0], k).bases(popcount(k)), k


def _polys(k, seed):
    """Montgomery bytes: uniform limbs below r, one value everywhere, and values from {0, 1, r - 1}"""
    rng = np.random.default_rng(seed)
    n = 1 << k
    a = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(n, 4), dtype=np.uint64)
    a[:, 3] = rng.integers(0, TOP_LIMB, size=n, dtype=np.uint64)
    x = int(rng.integers(1, 1 << 62))
    return [a.tobytes(), np.repeat(mont_rows([x]), n, axis=0).tobytes(),
            np.ascontiguousarray(mont_rows([0, 1, P - 1])[rng.integers(0, 3, size=n)]).tobytes()]


def _window_tables(hl, ctx, on):
    hl.set_option(ctx, "msm_window_tables", 17 if on else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("tables", [False, True], ids=["plain", "tables"])
@pytest.mark.parametrize("name", list(TRAPDOORS))
@pytest.mark.parametrize("k,nv", [pytest.param(6, 12, id="small-6"), pytest.param(12, 12, id="small-12"),
                                  pytest.param(16, 17, id="large-16")])
def test_commit_degenerate_trapdoor(hl, ctx, srs_cache, k, nv, name, tables):
    """commit / batch_commit = poly~(s) G: the polynomial's multilinear extension at the trapdoor (weights by popcount)"""
    ss, pp, _ = srs_cache(name, nv)
    ref = level_multiples(ss[0], k)
    pc = popcount(k)
    raws = _polys(k, 100 * k + nv)
    want = [ref.expected(r, pc) for r in raws]
    polys = [hl.MultilinearPolynomial(ctx, ctx.upload(r), k) for r in raws]
    _window_tables(hl, ctx, tables)
    try:
        assert [hl.MultilinearKzg.commit(pp, p) for p in polys] == want
        assert hl.MultilinearKzg.batch_commit(pp, polys) == want
        assert hl.MultilinearKzg.batch_commit(pp, polys[:2]) == want[:2]
    finally:
        _window_tables(hl, ctx, False)


@pytest.mark.gpu
@pytest.mark.parametrize("tables", [False, True], ids=["plain", "tables"])
@pytest.mark.parametrize("name", list(TRAPDOORS))
def test_open_degenerate_trapdoor_small(hl, ctx, srs_cache, name, tables):
    """open and batch_open at 2^12 are the C++ oracle's bytes, and the host verifier accepts them"""
    from oracle import cpu_oracle as co
    nv = 12
    ss, pp, flat = srs_cache(name, nv)
    vp = hl.MultilinearKzgVerifierParams.setup(ss)
    raws = _polys(nv, 7)
    polys = [hl.MultilinearPolynomial(ctx, ctx.upload(r), nv) for r in raws]
    _window_tables(hl, ctx, tables)
    try:
        # single opening
        t, ot = hl.Keccak256Transcript(), co.Transcript()
        comm = hl.MultilinearKzg.commit(pp, polys[0])
        t.write_commitment(comm), ot.write_commitment(comm)
        point = t.squeeze_challenges(nv)
        assert point == ot.squeeze_challenges(nv)
        ev = polys[0].evaluate(point)
        assert hl.MultilinearKzg.open(pp, polys[0], point, t) == ev == co.open_(ot, flat, nv, raws[0], point)
        proof = t.into_proof()
        assert proof == ot.into_proof()
        vt = hl.Keccak256Transcript.from_proof(proof)
        assert vt.read_commitment() == comm and vt.squeeze_challenges(nv) == point
        hl.mkzg_verify(vp, comm, point, ev, vt)
        # batch opening: three polys at two points
        pairs = [(0, 0), (1, 0), (2, 1), (0, 1)]
        t, ot = hl.Keccak256Transcript(), co.Transcript()
        comms = hl.MultilinearKzg.batch_commit_and_write(pp, polys, t)
        ot.write_commitments(comms)
        points = [t.squeeze_challenges(nv) for _ in range(2)]
        assert points == [ot.squeeze_challenges(nv) for _ in range(2)]
        vals = [polys[p].evaluate(points[q]) for p, q in pairs]
        t.write_field_elements(vals), ot.write_field_elements(vals)
        evs = [hl.Evaluation(p, q, v) for (p, q), v in zip(pairs, vals)]
        hl.MultilinearKzg.batch_open(pp, nv, polys, points, evs, t)
        co.batch_open(ot, flat, nv, nv, raws, points, hl._evaluations(evs), len(evs))
        proof = t.into_proof()
        assert proof == ot.into_proof()
        vt = hl.Keccak256Transcript.from_proof(proof)
        assert vt.read_commitments(3) == comms
        assert [vt.squeeze_challenges(nv) for _ in range(2)] == points
        assert vt.read_field_elements(len(vals)) == vals
        hl.mkzg_batch_verify(vp, nv, comms, points, evs, vt)
    finally:
        _window_tables(hl, ctx, False)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TRAPDOORS))
@pytest.mark.parametrize("n", [14, 17])
def test_lasso_degenerate_trapdoor(hl, ctx, srs_cache, name, n):
    """a Lasso proof of 2^n AND lookups over the degenerate SRS, window tables off and on: the C++ oracle's bytes, the
    derived (E) and packed (read_ts pair) commitments and the window-table jobs all over the degenerate points"""
    from oracle import cpu_oracle as co
    ss, pp, flat = srs_cache(name, 17)
    table = hl.LassoTable.bitwise(hl.SUBTABLE_AND, 4, 16)
    dims = [np.random.default_rng(170 + j).integers(0, 1 << 16, size=1 << n, dtype=np.uint32) for j in range(4)]
    ot = co.Transcript()
    co.lasso_prove(ot, flat, 17, table.to_c(), n, [d.tobytes() for d in dims])
    want = ot.into_proof()
    d_dims = [ctx.upload(d.tobytes()) for d in dims]
    for tables in (False, True):
        _window_tables(hl, ctx, tables)
        try:
            t = hl.Keccak256Transcript()
            hl.lasso_prove(pp, table, n, d_dims, t)
            route = hl.lasso_last_route(ctx)
        finally:
            _window_tables(hl, ctx, False)
        assert t.into_proof() == want, "window tables %s" % tables
        assert route["derived_commitments"] > 0 and route["packed_ts_pairs"] > 0, route
        assert (route["window_table_jobs"] > 0) == tables, route
    hl.lasso_verify(hl.MultilinearKzgVerifierParams.setup(ss), table, n, hl.Keccak256Transcript.from_proof(want))


# ------------------------------------------------------------------ forced MSM shapes
# one child process per set (the knobs are read once per process); LH_MSM_C_OFF = 12 - c puts the 2^12 cases at
# c = 5, 7, 11, 13, 17 (the 2^8 ones at c - 4, at least 4)
FORCED = [{"LH_MSM_C_OFF": "7", "LH_MSM_SEG": "16"},
          {"LH_MSM_C_OFF": "5", "LH_MSM_K2": "2"},
          {"LH_MSM_C_OFF": "1", "LH_MSM_HALF_MIN_LOG": "6"},
          {"LH_MSM_C_OFF": "-1", "LH_MSM_QUAD_MAX": "0"},
          {"LH_MSM_C_OFF": "-1", "LH_MSM_QUAD_MAX": "0", "LH_MSM_TREE_MAX": "0", "LH_MSM_TWO_LEVEL": "0"},
          {"LH_MSM_C_OFF": "-5", "LH_MSM_SEG": "4"}]


@pytest.mark.gpu
@pytest.mark.heavy(est=16)
def test_small_edges_under_forced_msm_shapes():
    """The `small` MSM and commit cases of this module again in child processes with the MSM's shape knobs forced:
    window widths 5, 7, 11, 13, 17; 16-bucket segments; continuation fan-in 2; every batch of two or more jobs as two
    pipelined halves (the batch commits); plain (not quad-cooperative) kernels at c = 13 with the two-level group
    reduction (4096 buckets per window: 1024 segments), and again with linear continuation levels and one-level
    reduction; 4-bucket segments at c = 17 (plain reduction, two levels, by size)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for env in FORCED:
        res = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_msm_edges.py", "-m", "gpu", "-x", "-q",
                              "-k", "small and (msm_fr or msm_u32 or distinct or commit) and not forced"], cwd=root, env=dict(os.environ, **env),
                             capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, (env, res.stdout[-3000:] + res.stderr[-2000:])
