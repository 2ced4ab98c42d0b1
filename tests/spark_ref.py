"""TEST INFRASTRUCTURE ONLY: Spark (Lasso paper, section 4; the sparse commitment of Spartan) - commit a sparse multilinear
polynomial once, prove its evaluations - on top of oracle/pyref (sum_check, gkr.prove_grand_product, kzg,
lasso.write_commitments / witness / _fingerprint).  This file is the specification of lh_spark_commit / lh_spark_open /
lh_spark_verify: the HIP prover reproduces these commitment and proof bytes.

Statement: a polynomial D in c l variables given by N = 2^n entries (dim_0[k], .., dim_{c-1}[k], val[k]), dim_j[k] < 2^l:
    D~(r_0, .., r_{c-1}) = sum_k val[k] prod_j eq(r_j, dim_j[k]),   r_j = point[j l .. (j + 1) l)
coordinate i of r_j belongs to bit i of dim_j; the dense index is sum_j dim_j << (j l); entries with the same index add up;
a caller pads with val = 0 entries.  nv = max(n, l).

Commit (no challenge, once): read_ts_j, final_cts_j as oracle.pyref.lasso.witness defines them; the commitment is the byte
string lasso.write_commitments makes on a fresh transcript of the 1 + 3 c polys [val | dim_j | read_ts_j | final_cts_j],
each zero-padded to nv: the mask element, then the non-identity points.

Open at `point` (transcript order == proof layout):

 0. C   n, l, c; the commitment's mask (common_field_element) and its points (common_commitment); the c l coordinates
 1.     T_j = eq_xy(r_j) (2^l entries), E_j[k] = T_j[dim_j[k]]
    W   ONE write_commitments block of E_0 .. E_{c-1}, padded to nv
 2. W   v = sum_k val[k] prod_j E_j[k]
 3.     ClassicSumCheck<EvaluationsProver> over n variables, expression Poly(0) Poly(1) .. Poly(c) over [val, E_0 ..], no eq
        factor, no ys, claim v -> r_z;   W  val(r_z), E_0(r_z) .. E_{c-1}(r_z)
 4. S   gamma, tau;  h(a, v, t) = a gamma^2 + v gamma + t - tau
        RS_j[k] = h(dim_j, E_j, read_ts_j), WS_j = RS_j + 1, Init_j[m] = h(m, T_j[m], 0), Final_j = Init_j + final_cts_j
 5.     gkr.prove_grand_product([RS_0, WS_0, .., RS_{c-1}, WS_{c-1}, Init_0, Final_0, ..]) -> r_N, r_M
 6. W   dim_j(r_N) | read_ts_j(r_N) | E_j(r_N) | final_cts_j(r_M)
 7.     ONE batch_open over nv variables: polys [val | dim | read_ts | final_cts | E] (commitment order, then E), points
        r_z, r_N, r_M zero-padded, evaluations (val, r_z), (E_j, r_z).., (dim_j, r_N).., (read_ts_j, r_N).., (E_j, r_N)..,
        (final_cts_j, r_M)..

The verifier mirrors this: v == value; the sum-check's final claim == val(r_z) prod E_j(r_z); Init_j WS_j = RS_j Final_j on
the roots; the leaf claims with T_j~(r_M) = eq_xy_eval(r_M, r_j) in closed form - it never sees a table; batch_verify over
commitment || E; no byte left.
"""
import random
import zlib

from oracle.pyref import expression as ex
from oracle.pyref import gkr, kzg
from oracle.pyref import lasso as o_lasso
from oracle.pyref import sum_check as sc
from oracle.pyref.field import R_MOD as P
from oracle.pyref.poly import eq_xy, eq_xy_eval, evaluate, identity_eval
from oracle.pyref.transcript import Keccak256Transcript

MAX_DIMS = 3
MAX_DIM_VARS = 24


class SparkError(Exception):
    pass


class _Spec:  # what lasso.witness reads of a table: its shape; no memories (E is the opening's business)
    def __init__(self, c, l):
        self.c, self.l, self.memories, self.alpha = c, l, [], 0

    def g_eval(self, vals):
        return 0


def _shape(n, l, c):
    if not 1 <= c <= MAX_DIMS:
        raise SparkError("num_dims out of range")
    if not 1 <= l <= MAX_DIM_VARS:
        raise SparkError("dim_vars out of range")
    if not 1 <= n < 31:
        raise SparkError("num_vars out of range")
    return max(n, l)


def num_committed(c):
    return 1 + 3 * c


def evaluations(c, v_rz, e_rz, dim_e, rts_e, e_rn, fc_e):
    """the opening list; polys: val 0 | dim 1.. | read_ts 1+c.. | final_cts 1+2c.. | E 1+3c..; points 0 = r_z, 1 = r_N, 2 = r_M"""
    out = [kzg.Evaluation(0, 0, v_rz)]
    out += [kzg.Evaluation(1 + 3 * c + j, 0, e_rz[j]) for j in range(c)]
    out += [kzg.Evaluation(1 + j, 1, dim_e[j]) for j in range(c)]
    out += [kzg.Evaluation(1 + c + j, 1, rts_e[j]) for j in range(c)]
    out += [kzg.Evaluation(1 + 3 * c + j, 1, e_rn[j]) for j in range(c)]
    out += [kzg.Evaluation(1 + 2 * c + j, 2, fc_e[j]) for j in range(c)]
    return out


class Committed:
    """the prover's handle: the entries, the counters, the commitments and the commitment bytes"""

    def __init__(self, n, l, dims, val, read_ts, final_cts, comms, blob):
        self.n, self.l, self.c = n, l, len(dims)
        self.dims, self.val, self.read_ts, self.final_cts, self.comms, self.blob = dims, val, read_ts, final_cts, comms, blob


def commit(pp, dims, val, l):
    """dims: c lists of 2^n ints below 2^l; val: 2^n field elements -> Committed"""
    N, c = len(val), len(dims)
    n = N.bit_length() - 1
    assert N == 1 << n and all(len(d) == N for d in dims)
    nv = _shape(n, l, c)
    if any(not 0 <= d < 1 << l for col in dims for d in col):
        raise SparkError("index out of range")
    w = o_lasso.witness(_Spec(c, l), dims)
    pp_nv = pp.trim(nv)
    polys = [[v % P for v in val]] + [list(d) for d in dims] + w["read_ts"] + w["final_cts"]
    comms = [kzg.commit(pp_nv, o_lasso._pad(p, nv)) for p in polys]
    t = Keccak256Transcript()
    o_lasso.write_commitments(t, comms)
    return Committed(n, l, [list(d) for d in dims], [v % P for v in val], w["read_ts"], w["final_cts"], comms, t.into_proof())


def _header(transcript, n, l, c, mask, points, point):
    transcript.common_field_elements([n, l, c])
    transcript.common_field_element(mask)
    for cm in points:
        transcript.common_commitment(cm)
    transcript.common_field_elements(point)


def open_(pp, cm, point, transcript, forge=None):
    """-> the value D~(point); the proof is appended to `transcript`.
    forge (tests only): called with the honest memories E (c lists), returns the ones a cheating prover goes on with."""
    n, l, c = cm.n, cm.l, cm.c
    N, M = 1 << n, 1 << l
    nv = _shape(n, l, c)
    assert len(point) == c * l
    mask = sum(1 << i for i, x in enumerate(cm.comms) if x is None)
    _header(transcript, n, l, c, mask, [x for x in cm.comms if x is not None], point)
    pp_nv = pp.trim(nv)
    T = [eq_xy(point[j * l:(j + 1) * l]) for j in range(c)]
    E = [[T[j][d] for d in cm.dims[j]] for j in range(c)]
    if forge:
        E = forge(E)
    o_lasso.write_commitments(transcript, [kzg.commit(pp_nv, o_lasso._pad(e, nv)) for e in E])
    v = 0
    for k in range(N):
        t = cm.val[k]
        for j in range(c):
            t = t * E[j][k] % P
        v = (v + t) % P
    transcript.write_field_element(v)
    expr = ex.Poly(0)
    for i in range(1, c + 1):
        expr = expr * ex.Poly(i)
    r_z, at_rz = sc.prove(sc.EvaluationsProver, n, sc.VirtualPolynomial(expr, [cm.val] + E, [], []), v, transcript)
    transcript.write_field_elements(at_rz)

    gamma = transcript.squeeze_challenge()
    tau = transcript.squeeze_challenge()
    h = o_lasso._fingerprint
    leaves_n, leaves_l = [], []
    for j in range(c):
        rs = [h(cm.dims[j][k], E[j][k], cm.read_ts[j][k], gamma, tau) for k in range(N)]
        init = [h(m, T[j][m], 0, gamma, tau) for m in range(M)]
        leaves_n += [rs, [(x + 1) % P for x in rs]]
        leaves_l += [init, [(init[m] + cm.final_cts[j][m]) % P for m in range(M)]]
    _, claims = gkr.prove_grand_product(leaves_n + leaves_l, transcript)
    r_N, r_M = claims[0][1], claims[2 * c][1]

    dim_e = [evaluate(t, r_N) for t in cm.dims]
    rts_e = [evaluate(t, r_N) for t in cm.read_ts]
    e_rn = [evaluate(t, r_N) for t in E]
    fc_e = [evaluate(t, r_M) for t in cm.final_cts]
    transcript.write_field_elements(dim_e + rts_e + e_rn + fc_e)
    polys = [o_lasso._pad(p, nv) for p in [cm.val] + cm.dims + cm.read_ts + cm.final_cts + E]
    points = [o_lasso._pad_point(pt, nv) for pt in (r_z, r_N, r_M)]
    kzg.batch_open(pp_nv, nv, polys, points, evaluations(c, at_rz[0], at_rz[1:], dim_e, rts_e, e_rn, fc_e), transcript)
    return v


def read_commitment_blob(blob, c):
    """-> (mask, comms with None for the identity): the blob is a transcript's stream of its own"""
    t = Keccak256Transcript(blob)
    try:
        comms = o_lasso.read_commitments(t, num_committed(c))
    except Exception as e:
        raise SparkError("malformed commitment: %s" % e)
    if t.pos != len(t.stream):
        raise SparkError("malformed commitment: wrong length")
    return sum(1 << i for i, x in enumerate(comms) if x is None), comms


def verify(vp, n, l, c, blob, point, value, transcript):
    """Raises on any proof that does not verify."""
    nv = _shape(n, l, c)
    assert len(point) == c * l
    mask, comms = read_commitment_blob(blob, c)
    _header(transcript, n, l, c, mask, [x for x in comms if x is not None], point)
    comms = comms + o_lasso.read_commitments(transcript, c)
    v = transcript.read_field_element()
    if v != value % P:
        raise SparkError("the proof is of another value")
    final, r_z = sc.verify(sc.Evaluations, n, c + 1, v, transcript)
    at_rz = transcript.read_field_elements(c + 1)
    prod = 1
    for x in at_rz:
        prod = prod * x % P
    if prod != final:
        raise SparkError("sum-check final evaluation mismatch")
    gamma = transcript.squeeze_challenge()
    tau = transcript.squeeze_challenge()
    roots, claims = gkr.verify_grand_product([n] * (2 * c) + [l] * (2 * c), transcript)
    for j in range(c):
        if roots[2 * c + 2 * j] * roots[2 * j + 1] % P != roots[2 * j] * roots[2 * c + 2 * j + 1] % P:
            raise SparkError("dimension %d: Init*WS != RS*Final" % j)
    r_N, r_M = claims[0][1], claims[2 * c][1]
    vals = transcript.read_field_elements(4 * c)
    dim_e, rts_e, e_rn, fc_e = vals[:c], vals[c:2 * c], vals[2 * c:3 * c], vals[3 * c:]
    h = o_lasso._fingerprint
    id_M = identity_eval(r_M)
    for j in range(c):
        rs = h(dim_e[j], e_rn[j], rts_e[j], gamma, tau)
        init = h(id_M, eq_xy_eval(r_M, point[j * l:(j + 1) * l]), 0, gamma, tau)
        want = [rs, (rs + 1) % P, init, (init + fc_e[j]) % P]
        got = [claims[2 * j][0], claims[2 * j + 1][0], claims[2 * c + 2 * j][0], claims[2 * c + 2 * j + 1][0]]
        if want != got:
            raise SparkError("dimension %d: leaf claim mismatch" % j)
    points = [o_lasso._pad_point(pt, nv) for pt in (r_z, r_N, r_M)]
    kzg.batch_verify(vp.trim(nv), nv, comms, points, evaluations(c, at_rz[0], at_rz[1:], dim_e, rts_e, e_rn, fc_e), transcript)
    if transcript.pos != len(transcript.stream):
        raise SparkError("trailing bytes in proof")


# ------------------------------------------------------------------ two independent statements of the value
def sparse_eval(dims, val, l, point):
    """the defining sum, eq factor by factor: no table"""
    total = 0
    for k in range(len(val)):
        t = val[k] % P
        for j, col in enumerate(dims):
            d = col[k]
            for i in range(l):
                x = point[j * l + i]
                t = t * (x if (d >> i) & 1 else 1 - x) % P
        total = (total + t) % P
    return total


def dense_eval(dims, val, l, point):
    """the dense table of 2^(c l) entries (index sum_j dim_j << (j l), equal indices add up), evaluated"""
    c = len(dims)
    table = [0] * (1 << (c * l))
    for k in range(len(val)):
        at = sum(dims[j][k] << (j * l) for j in range(c))
        table[at] = (table[at] + val[k]) % P
    return evaluate(table, point)


# ------------------------------------------------------------------ the named cases: (n, l, c)
CASES = {
    "one_var": (1, 1, 1),
    "matrix": (5, 3, 2),
    "big_dims": (2, 4, 2),
    "vector": (6, 6, 1),
    "cube": (4, 2, 3),
    "one_index": (4, 3, 2),
    "distinct": (3, 4, 2),
    "zero_val": (3, 2, 2),
    "duplicates": (3, 2, 2),
    "boolean_point": (4, 3, 2),
    "two_points": (5, 3, 2),
    "mid": (13, 9, 2),
    "wide": (9, 12, 1),
}
SMALL = [k for k in CASES if max(CASES[k][:2]) <= 6]  # the cases the golden SRS of six variables covers


def _rng(case, what):
    return random.Random(zlib.crc32(repr(("spark", case, what)).encode()))


def case_entries(case):
    """-> (dims, val): c lists of 2^n indices, 2^n field elements"""
    n, l, c = CASES[case]
    N, M = 1 << n, 1 << l
    rng = _rng(case, "entries")
    dims = [[rng.randrange(M) for _ in range(N)] for _ in range(c)]
    val = [rng.randrange(P) for _ in range(N)]
    if case == "one_index":
        dims = [[5] * N for _ in range(c)]
    if case == "distinct":
        dims = [rng.sample(range(M), N) for _ in range(c)]
    if case == "zero_val":
        val = [0] * N
    if case == "duplicates":
        dims = [col[:N // 2] * 2 for col in dims]
    return dims, val


def case_points(case):
    """the points the golden file records openings at"""
    n, l, c = CASES[case]
    rng = _rng(case, "points")
    count = 2 if case == "two_points" else 1
    points = [[rng.randrange(P) for _ in range(c * l)] for _ in range(count)]
    if case == "boolean_point":  # the index tuple of entry 3
        dims, _ = case_entries(case)
        points = [[(dims[j][3] >> i) & 1 for j in range(c) for i in range(l)]]
    return points


# ------------------------------------------------------------------ forgeries: (n, l, c, dims, val, point, forge)
def forgery(name):
    if name == "bad_e":
        dims, val = [[0, 1, 1, 0], [1, 1, 0, 1]], [3, 5, 7, 11]
        point = [0x1234567, 0x89ABCDE]

        def forge(E):
            E = [list(e) for e in E]
            E[0][0] = (E[0][0] + 1) % P
            return E

        return 2, 1, 2, dims, val, point, forge
    raise KeyError(name)


FORGERIES = {"bad_e": r"Init\*WS != RS\*Final"}
