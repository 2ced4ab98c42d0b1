"""TEST INFRASTRUCTURE ONLY: Spartan - R1CS satisfiability over Spark-committed matrices - on top of oracle/pyref
(sum_check, kzg, lasso.write_commitments) and tests/spark_ref.py (commit, open_, verify), both unchanged.  This file is the
specification of lh_r1cs_commit / lh_spartan_prove / lh_spartan_verify: the HIP prover reproduces these key and proof bytes.

Statement: matrices A, B, C of 2^l x 2^l, each given by N = 2^n entries (row[k], col[k], val[k]) with row, col < 2^l (the same
n for the three; equal positions add up; pad with val = 0).  z has 2^l entries: z[y] = w[y] for y < 2^(l-1) (the witness),
z[2^(l-1) + i] = x[i] for i < p (the public input, 1 <= p <= 2^(l-1); the constant 1 is the caller's x[0]), 0 above.
Satisfied: (Az)[i] (Bz)[i] = (Cz)[i] for every row i.  Spark convention: dim_0 = row, dim_1 = col, c = 2; coordinate i of a
point belongs to bit i of the index, so the witness / public split is coordinate l - 1 of r_y.

Key (no challenge, once): spark_ref.commit of A, B, C; the key blob is the three commitment blobs one after the other.

Prove (transcript order == proof layout):

 0. C   n, l, p; per matrix its commitment's mask (common_field_element) and its points (common_commitment); x[0..p)
 1. W   ONE write_commitments block of w (l - 1 variables): the mask element, the point unless w is zero
 2. S   tau (l elements)
 3.     Az, Bz, Cz (a witness that does not satisfy the instance is refused BEFORE step 0: nothing is written)
 4.     outer: ClassicSumCheck<EvaluationsProver> over l variables, EqXY(0) (Poly(0) Poly(1) - Poly(2)) over [Az, Bz, Cz],
        ys = [tau], claim 0 -> r_x;   W  vA, vB, vC = Az~(r_x), Bz~(r_x), Cz~(r_x)
 5. S   rho;  T = vA + rho vB + rho^2 vC
 6.     M_A[y] = sum_{k: colA[k] = y} valA[k] eq(r_x, rowA[k]), likewise M_B, M_C
 7.     inner: EvaluationsProver over l variables, Poly(0) Poly(3) + rho Poly(1) Poly(3) + rho^2 Poly(2) Poly(3) over
        [M_A, M_B, M_C, z], no eq factor, claim T -> r_y;   W  eA, eB, eC = M_.(r_y);   W  e_w = w~(r_y[0 .. l-1))
 8.     batch_open over l - 1 variables: one poly (w), one point (r_y[0 .. l-1)), value e_w.  batch_open takes at least two
        evaluations (eq_xy of an empty point is the zero poly), so the one evaluation is listed TWICE: the merged poly is
        ((1 - t) + t) w = w
 9.     spark_ref.open_ of A, then B, then C at r_x || r_y on the same transcript; the values are eA, eB, eC

Verify mirrors it: the outer final claim == eq(tau, r_x) (vA vB - vC); z~(r_y) = (1 - r_y[l-1]) e_w + r_y[l-1] x~(r_y[0..l-1))
with x~ at a cost that follows p (x padded to 2^q, the first q coordinates, times prod_{q <= i < l-1} (1 - r_i)); the inner
final claim == (eA + rho eB + rho^2 eC) z~(r_y); the opening of w; spark verify three times; no byte left.
"""
import random
import zlib

import spark_ref as spr
from oracle.pyref import expression as ex
from oracle.pyref import kzg
from oracle.pyref import lasso as o_lasso
from oracle.pyref import sum_check as sc
from oracle.pyref.field import R_MOD as P
from oracle.pyref.poly import eq_xy, eq_xy_eval, evaluate

MIN_DIM_VARS = 2
MAX_DIM_VARS = spr.MAX_DIM_VARS
TILE = 4096  # the most entries a workgroup of spartan_spmv takes (csrc/kernels_spartan.hip SPMV_TILE is at most this)


class SpartanError(Exception):
    pass


def _shape(n, l, p):
    """-> the SRS variables the argument needs"""
    if not MIN_DIM_VARS <= l <= MAX_DIM_VARS:
        raise SpartanError("dim_vars out of range")
    if not 1 <= n < 31:
        raise SpartanError("num_vars out of range")
    if not 1 <= p <= 1 << (l - 1):
        raise SpartanError("num_public out of range")
    return max(n, l)


class Key:
    """the three committed matrices (spark_ref.Committed, dims = [row, col]) and the key blob"""

    def __init__(self, n, l, mats):
        self.n, self.l, self.mats = n, l, mats
        self.blob = b"".join(m.blob for m in mats)


def commit(pp, instance, l):
    """instance: three (row, col, val) of 2^n entries each -> Key"""
    n = len(instance[0][2]).bit_length() - 1
    if any(len(col) != 1 << n for m in instance for col in m):
        raise SpartanError("matrices of 2^num_vars entries, the same for the three")
    _shape(n, l, 1)
    try:
        return Key(n, l, [spr.commit(pp, [row, col], val, l) for row, col, val in instance])
    except spr.SparkError as e:
        raise SpartanError(str(e))


def split_key(blob):
    """-> the three Spark commitment blobs; each is its mask element and its non-identity points"""
    out, at = [], 0
    for _ in range(3):
        if len(blob) < at + 32:
            raise SpartanError("malformed key: too short")
        mask = int.from_bytes(blob[at:at + 32], "big")
        if mask >> spr.num_committed(2):
            raise SpartanError("malformed key: commitment mask out of range")
        size = 32 + 64 * (spr.num_committed(2) - bin(mask).count("1"))
        if len(blob) < at + size:
            raise SpartanError("malformed key: too short")
        out.append(blob[at:at + size])
        at += size
    if at != len(blob):
        raise SpartanError("malformed key: wrong length")
    return out


def assignment(l, w, x):
    half = 1 << (l - 1)
    assert len(w) == half and 1 <= len(x) <= half
    return [v % P for v in w] + [v % P for v in x] + [0] * (half - len(x))


def spmv(seg, other, val, X, size):
    """the keyed field sum: out[s] = sum_{k: seg[k] = s} val[k] X[other[k]]"""
    out = [0] * size
    for s, o, v in zip(seg, other, val):
        out[s] = (out[s] + v * X[o]) % P
    return out


def satisfied(instance, w, x, l):
    """from the dense matrices: independent of the sparse path.  -> the number of rows with Az Bz != Cz"""
    M = 1 << l
    z = assignment(l, w, x)
    prods = []
    for row, col, val in instance:
        dense = [[0] * M for _ in range(M)]
        for r, c, v in zip(row, col, val):
            dense[r][c] = (dense[r][c] + v) % P
        prods.append([sum(a * b for a, b in zip(dense[i], z)) % P for i in range(M)])
    return sum(1 for i in range(M) if (prods[0][i] * prods[1][i] - prods[2][i]) % P)


def _header(transcript, n, l, p, comm_lists, x):
    transcript.common_field_elements([n, l, p])
    for comms in comm_lists:
        transcript.common_field_element(sum(1 << i for i, cm in enumerate(comms) if cm is None))
        for cm in comms:
            if cm is not None:
                transcript.common_commitment(cm)
    transcript.common_field_elements([v % P for v in x])


def _outer_expression():
    return ex.EqXY(0) * (ex.Poly(0) * ex.Poly(1) - ex.Poly(2))


def _inner_expression(rho):
    return ex.Poly(0) * ex.Poly(3) + ex.Poly(1) * ex.Poly(3) * rho + ex.Poly(2) * ex.Poly(3) * (rho * rho % P)


def _w_evaluations(e_w):
    return [kzg.Evaluation(0, 0, e_w), kzg.Evaluation(0, 0, e_w)]


def public_eval(x, point):
    """x~ over len(point) variables (x zero-padded) at a cost that follows len(x)"""
    q = (len(x) - 1).bit_length()
    v = evaluate([t % P for t in x] + [0] * ((1 << q) - len(x)), point[:q]) if q else x[0] % P
    for r in point[q:]:
        v = v * (1 - r) % P
    return v


def prove(pp, key, w, x, transcript, forge=None):
    """Appends the proof to `transcript`.  forge (tests only): "bad_witness" goes on with a w that does not satisfy the
    instance; "bad_eval" writes eA + 1."""
    n, l, p = key.n, key.l, len(x)
    _shape(n, l, p)
    M = 1 << l
    z = assignment(l, w, x)
    mats = [(m.dims[0], m.dims[1], m.val) for m in key.mats]
    Mz = [spmv(row, col, val, z, M) for row, col, val in mats]
    bad = sum(1 for i in range(M) if (Mz[0][i] * Mz[1][i] - Mz[2][i]) % P)
    if bad and forge != "bad_witness":
        raise SpartanError("the witness does not satisfy %d of the 2^%d constraints" % (bad, l))
    _header(transcript, n, l, p, [m.comms for m in key.mats], x)
    w = [v % P for v in w]
    pp_w = pp.trim(l - 1)
    cw = kzg.commit(pp_w, w)
    o_lasso.write_commitments(transcript, [cw])
    tau = transcript.squeeze_challenges(l)
    r_x, at_rx = sc.prove(sc.EvaluationsProver, l, sc.VirtualPolynomial(_outer_expression(), Mz, [], [tau]), 0, transcript)
    transcript.write_field_elements(at_rx)
    rho = transcript.squeeze_challenge()
    T = (at_rx[0] + rho * at_rx[1] + rho * rho % P * at_rx[2]) % P
    eq_rx = eq_xy(r_x)
    Mc = [spmv(col, row, val, eq_rx, M) for row, col, val in mats]
    r_y, at_ry = sc.prove(sc.EvaluationsProver, l, sc.VirtualPolynomial(_inner_expression(rho), Mc + [z], [], []), T, transcript)
    e = list(at_ry[:3])
    if forge == "bad_eval":
        e[0] = (e[0] + 1) % P
    transcript.write_field_elements(e)
    e_w = evaluate(w, r_y[:l - 1])
    transcript.write_field_element(e_w)
    kzg.batch_open(pp_w, l - 1, [w], [r_y[:l - 1]], _w_evaluations(e_w), transcript)
    for m, want in zip(key.mats, at_ry[:3]):
        v = spr.open_(pp, m, r_x + r_y, transcript)
        assert v == want


def _spark_verify_midstream(vp, n, l, blob, point, value, transcript, last):
    """spark_ref.verify ends by refusing bytes it has not read; here the next opening follows on the same transcript.
    That check is its last statement, so for all but the last opening this one refusal means "verified, bytes follow"."""
    try:
        spr.verify(vp, n, l, 2, blob, point, value, transcript)
    except spr.SparkError as e:
        if last or str(e) != "trailing bytes in proof":
            raise SpartanError(str(e))


def verify(vp, n, l, blob, x, transcript):
    """Raises SpartanError on any proof that does not verify (a piece's own refusal keeps its words)."""
    try:
        _verify(vp, n, l, blob, x, transcript)
    except (sc.SumCheckError, kzg.PcsError, o_lasso.LassoError) as e:
        raise SpartanError(str(e))


def _verify(vp, n, l, blob, x, transcript):
    p = len(x)
    _shape(n, l, p)
    blobs = split_key(blob)
    try:
        comm_lists = [spr.read_commitment_blob(b, 2)[1] for b in blobs]
    except spr.SparkError as e:
        raise SpartanError("malformed key: %s" % e)
    _header(transcript, n, l, p, comm_lists, x)
    cw = o_lasso.read_commitments(transcript, 1)
    tau = transcript.squeeze_challenges(l)
    final, r_x = sc.verify(sc.Evaluations, l, 3, 0, transcript)
    vA, vB, vC = transcript.read_field_elements(3)
    if final != eq_xy_eval(tau, r_x) * (vA * vB - vC) % P:
        raise SpartanError("outer sum-check final evaluation mismatch")
    rho = transcript.squeeze_challenge()
    T = (vA + rho * vB + rho * rho % P * vC) % P
    final, r_y = sc.verify(sc.Evaluations, l, 2, T, transcript)
    eA, eB, eC = transcript.read_field_elements(3)
    e_w = transcript.read_field_element()
    top = r_y[l - 1]
    z_ry = ((1 - top) * e_w + top * public_eval(x, r_y[:l - 1])) % P
    if final != (eA + rho * eB + rho * rho % P * eC) * z_ry % P:
        raise SpartanError("inner sum-check final evaluation mismatch")
    kzg.batch_verify(vp.trim(l - 1), l - 1, cw, [r_y[:l - 1]], _w_evaluations(e_w), transcript)
    for i, (b, value) in enumerate(zip(blobs, (eA, eB, eC))):
        _spark_verify_midstream(vp, n, l, b, r_x + r_y, value, transcript, i == 2)
    if transcript.pos != len(transcript.stream):
        raise SpartanError("trailing bytes in proof")


# ------------------------------------------------------------------ the named cases: (n, l, p)
CASES = {
    "tiny": (1, 2, 1),
    "square": (3, 3, 2),
    "many": (5, 3, 2),
    "tall": (2, 4, 3),
    "one_segment": (4, 3, 1),
    "zero_c": (3, 3, 1),
    "full_public": (3, 3, 4),
    "two_witnesses": (3, 3, 2),
    "mid": (12, 10, 5),
}
SMALL = [k for k in CASES if max(CASES[k][:2]) <= 6]  # the cases the golden SRS of six variables covers


def _rng(case, what):
    return random.Random(zlib.crc32(repr(("spartan", case, what)).encode()))


def _close(A, B, w, x, n, l):
    """C for the given A, B and assignment: the entry of every row A uses, in the constant column (index 2^(l-1), where
    x[0] = 1 lives), is (Az)[i] (Bz)[i]; a row A does not use has (Az)[i] = 0.  Padded with val = 0 entries."""
    N, M, half = 1 << n, 1 << l, 1 << (l - 1)
    z = assignment(l, w, x)
    Az, Bz = spmv(A[0], A[1], A[2], z, M), spmv(B[0], B[1], B[2], z, M)
    rows = sorted(set(A[0]))
    pad = [0] * (N - len(rows))
    return (rows + pad, [half] * N, [Az[i] * Bz[i] % P for i in rows] + pad)


def satisfiable(rng, n, l, p, a_rows=None, a_cols=None, b_cols=None, a_zero=False, duplicates=False):
    """-> (instance, w, x): A, B and z drawn at random, C closed over them (_close); x[0] = 1.
    a_rows / b_cols: one index for every entry of A's rows / B's columns; a_cols, with b_cols None: the columns A and B draw from"""
    N, M, half = 1 << n, 1 << l, 1 << (l - 1)
    draw = lambda fixed, among=None: [fixed if fixed is not None else (rng.choice(among) if among else rng.randrange(M))
                                      for _ in range(N)]
    A = [draw(a_rows), draw(None, a_cols), [0 if a_zero else rng.randrange(P) for _ in range(N)]]
    B = [draw(None), draw(b_cols, a_cols), [rng.randrange(P) for _ in range(N)]]
    if duplicates:  # every position twice
        for m in (A, B):
            m[0], m[1] = m[0][:N // 2] * 2, m[1][:N // 2] * 2
    w = [rng.randrange(P) for _ in range(half)]
    x = [1] + [rng.randrange(P) for _ in range(p - 1)]
    A, B = tuple(A), tuple(B)
    return [A, B, _close(A, B, w, x, n, l)], w, x


def case_instance(case):
    """-> (instance, [(w, x), ..]): the assignments the golden file records proofs of"""
    n, l, p = CASES[case]
    rng = _rng(case, "instance")
    half = 1 << (l - 1)
    kw = {}
    if case == "one_segment":
        kw = dict(a_rows=5, b_cols=half)
    if case == "zero_c":
        kw = dict(a_zero=True)
    if case == "many":
        kw = dict(duplicates=True)
    if case == "two_witnesses":  # A and B read w[0], w[1] and the public half only: w[2], w[3] are free
        kw = dict(a_cols=[0, 1, half, half + 1])
    inst, w, x = satisfiable(rng, n, l, p, **kw)
    assigns = [(w, x)]
    if case == "two_witnesses":
        assigns.append((w[:2] + [rng.randrange(P), rng.randrange(P)], x))
    return inst, assigns


# ------------------------------------------------------------------ forgeries: name -> the verifier's words
FORGERIES = {
    "bad_witness": "outer sum-check final evaluation mismatch",
    "bad_eval": "inner sum-check final evaluation mismatch",
    "bad_public": "Consistency failure at round 1",  # (x is absorbed: every challenge differs, round 0 still claims 0)
}


def forgery(name):
    """-> (case, w, x_proved, x_verified, forge): all on `square`'s instance"""
    inst, assigns = case_instance("square")
    w, x = assigns[0]
    if name == "bad_witness":
        # the first w entry whose change fails exactly one row
        l = CASES["square"][1]
        for y in range(len(w)):
            w2 = list(w)
            w2[y] = (w2[y] + 1) % P
            if satisfied(inst, w2, x, l) == 1:
                return "square", w2, x, x, "bad_witness"
        raise AssertionError("no witness entry fails exactly one row")
    if name == "bad_eval":
        return "square", w, x, x, "bad_eval"
    if name == "bad_public":
        return "square", w, x, [x[0], (x[1] + 1) % P], None
    raise KeyError(name)
