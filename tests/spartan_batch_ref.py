"""TEST INFRASTRUCTURE ONLY: batched Spartan - K' assignments of ONE R1CS key in one proof - on top of oracle/pyref,
tests/spark_ref.py and tests/spartan_ref.py (and tests/nova_ref.py's circuit for instances), all unchanged.  This file is the
specification of batched Spartan: lh_spartan_verify_batch accepts these proof bytes (the library has no device prover for
them yet: DESIGN.md section 27).

Statement: a key (n, l) of spartan_ref.commit; K' >= 2 instances, k = ceil(log2 K'), K = 2^k, l + k <= MAX_BATCH_VARS; every
instance has p public inputs.  Instance i < K' has z_i = (w_i, x_i, 0) in spartan_ref's layout; instances K' <= i < K are zero
(z = 0 satisfies every R1CS).  Coordinate i of a point belongs to bit i of the index, and the instance index takes the LOW k
bits of every stacked table: Z[i + K y], MZ_m[i + K s] = (M_m z_i)[s], W[i + K y] for y < 2^(l-1) (the first K 2^(l-1)
elements of Z).

Prove (transcript order == proof layout):

 0. C   n, l, p and the key as spartan_ref._header does; K'; the K' p public inputs, instance by instance
 1. W   ONE write_commitments block of W (k + l - 1 variables)
 2. S   tau (k + l elements)
 3.     Z, MZ_A, MZ_B, MZ_C; a batch that does not satisfy is refused BEFORE step 0: nothing is written
 4.     outer: spartan_ref's expression over k + l variables and [MZ_A, MZ_B, MZ_C], ys = [tau], claim 0 -> r = r_b || r_x;
        W  vA, vB, vC = the stacked tables at r
 5. S   rho;  T = vA + rho vB + rho^2 vC;  zbar[y] = sum_i eq(r_b, i) Z[i + K y]
 6.     M_A, M_B, M_C bound at r_x, as spartan_ref's step 6
 7.     inner: spartan_ref's expression over l variables and [M_A, M_B, M_C, zbar], claim T -> r_y;  W  eA, eB, eC;
        W  e_w = W~(r_b || r_y[0 .. l-1))
 8.     batch_open over k + l - 1 variables: W at that point, the evaluation listed twice (spartan_ref step 8)
 9.     spark_ref.open_ of A, B, C at r_x || r_y

Verify mirrors it: the outer final claim == eq(tau, r) (vA vB - vC); xbar[j] = sum_{i < K'} eq(r_b, i) x_i[j];
zbar~(r_y) = (1 - r_y[l-1]) e_w + r_y[l-1] xbar~(r_y[0..l-1)); the inner final claim; the opening of W; spark verify three
times; no byte left.
"""
import random
import zlib

import nova_ref as nv
import spark_ref as spr
import spartan_ref as spa
from oracle.pyref import kzg
from oracle.pyref import lasso as o_lasso
from oracle.pyref import sum_check as sc
from oracle.pyref.field import R_MOD as P
from oracle.pyref.poly import eq_xy, eq_xy_eval, evaluate

MAX_BATCH_VARS = 26


def batch_vars(count):
    return (count - 1).bit_length()


def _shape(n, l, p, count):
    """-> (k, the SRS variables the argument needs)"""
    spa._shape(n, l, p)
    if count < 2:
        raise spa.SpartanError("num_instances out of range (at least 2)")
    k = batch_vars(count)
    if l + k > MAX_BATCH_VARS:
        raise spa.SpartanError("dim_vars + batch_vars out of range (at most %d)" % MAX_BATCH_VARS)
    return k, max(n, k + l - 1)


def stack(vectors, k):
    """instance-minor: out[i + K y] = vectors[i][y]; the instances beyond len(vectors) are zero"""
    K, size = 1 << k, len(vectors[0])
    out = [0] * (K * size)
    for i, v in enumerate(vectors):
        out[i::K] = [t % P for t in v]
    return out


def assignment(l, ws, xs):
    """-> Z of 2^(k + l) entries"""
    return stack([spa.assignment(l, w, x) for w, x in zip(ws, xs)], batch_vars(len(ws)))


def spmv_batch(seg, other, val, Z, size, K):
    """the keyed field sum over K right-hand sides: out[i + K s] = sum_{j: seg[j] = s} val[j] Z[i + K other[j]]"""
    out = [0] * (size * K)
    for s, o, v in zip(seg, other, val):
        if v:
            for i in range(K):
                out[i + K * s] = (out[i + K * s] + v * Z[i + K * o]) % P
    return out


def combine(Z, r_b, l):
    """zbar[y] = sum_i eq(r_b, i) Z[i + K y]"""
    K, e = 1 << len(r_b), eq_xy(r_b)
    return [sum(a * b for a, b in zip(e, Z[K * y:K * y + K])) % P for y in range(1 << l)]


def unsatisfied(MZ, K):
    """-> (the number of rows of the stacked tables with Az Bz != Cz, the lowest instance with one or None)"""
    bad = [j for j, (a, b, c) in enumerate(zip(*MZ)) if (a * b - c) % P]
    return len(bad), (min(j % K for j in bad) if bad else None)


def satisfied(instance, ws, xs, l):
    """from the dense matrices -> (the rows that fail over all instances, the lowest failing instance or None)"""
    counts = [spa.satisfied(instance, w, x, l) for w, x in zip(ws, xs)]
    failing = [i for i, c in enumerate(counts) if c]
    return sum(counts), (failing[0] if failing else None)


def _header(transcript, n, l, p, comm_lists, xs):
    spa._header(transcript, n, l, p, comm_lists, [])
    transcript.common_field_element(len(xs))
    for x in xs:
        transcript.common_field_elements([v % P for v in x])


def prove(pp, key, ws, xs, transcript, forge=None):
    """Appends the proof to `transcript`.  forge (tests only): "bad_witness" goes on with a batch that does not satisfy;
    "bad_eval" writes eA + 1."""
    n, l, p, count = key.n, key.l, len(xs[0]), len(ws)
    if len(xs) != count or any(len(x) != p for x in xs):
        raise spa.SpartanError("as many public inputs as witnesses, num_public each")
    k, _ = _shape(n, l, p, count)
    K, M, half = 1 << k, 1 << l, 1 << (l - 1)
    Z = assignment(l, ws, xs)
    mats = [(m.dims[0], m.dims[1], m.val) for m in key.mats]
    MZ = [spmv_batch(row, col, val, Z, M, K) for row, col, val in mats]
    bad, first = unsatisfied(MZ, K)
    if bad and forge != "bad_witness":
        raise spa.SpartanError("the batch does not satisfy %d of its constraints (first: instance %d)" % (bad, first))
    _header(transcript, n, l, p, [m.comms for m in key.mats], xs)
    W = Z[:K * half]
    pp_w = pp.trim(k + l - 1)
    o_lasso.write_commitments(transcript, [kzg.commit(pp_w, W)])
    tau = transcript.squeeze_challenges(k + l)
    r, at_r = sc.prove(sc.EvaluationsProver, k + l, sc.VirtualPolynomial(spa._outer_expression(), MZ, [], [tau]), 0, transcript)
    r_b, r_x = r[:k], r[k:]
    transcript.write_field_elements(at_r)
    rho = transcript.squeeze_challenge()
    T = (at_r[0] + rho * at_r[1] + rho * rho % P * at_r[2]) % P
    zbar = combine(Z, r_b, l)
    eq_rx = eq_xy(r_x)
    Mc = [spa.spmv(col, row, val, eq_rx, M) for row, col, val in mats]
    r_y, at_ry = sc.prove(sc.EvaluationsProver, l, sc.VirtualPolynomial(spa._inner_expression(rho), Mc + [zbar], [], []), T, transcript)
    e = list(at_ry[:3])
    if forge == "bad_eval":
        e[0] = (e[0] + 1) % P
    transcript.write_field_elements(e)
    point = r_b + r_y[:l - 1]
    e_w = evaluate(W, point)
    transcript.write_field_element(e_w)
    kzg.batch_open(pp_w, k + l - 1, [W], [point], spa._w_evaluations(e_w), transcript)
    for m, want in zip(key.mats, at_ry[:3]):
        v = spr.open_(pp, m, r_x + r_y, transcript)
        assert v == want


def verify(vp, n, l, blob, xs, transcript):
    """Raises SpartanError on any proof that does not verify (a piece's own refusal keeps its words)."""
    try:
        _verify(vp, n, l, blob, xs, transcript)
    except (sc.SumCheckError, kzg.PcsError, o_lasso.LassoError) as e:
        raise spa.SpartanError(str(e))


def _verify(vp, n, l, blob, xs, transcript):
    p, count = len(xs[0]), len(xs)
    if any(len(x) != p for x in xs):
        raise spa.SpartanError("num_public public inputs per instance")
    k, _ = _shape(n, l, p, count)
    blobs = spa.split_key(blob)
    try:
        comm_lists = [spr.read_commitment_blob(b, 2)[1] for b in blobs]
    except spr.SparkError as e:
        raise spa.SpartanError("malformed key: %s" % e)
    _header(transcript, n, l, p, comm_lists, xs)
    cw = o_lasso.read_commitments(transcript, 1)
    tau = transcript.squeeze_challenges(k + l)
    final, r = sc.verify(sc.Evaluations, k + l, 3, 0, transcript)
    r_b, r_x = r[:k], r[k:]
    vA, vB, vC = transcript.read_field_elements(3)
    if final != eq_xy_eval(tau, r) * (vA * vB - vC) % P:
        raise spa.SpartanError("outer sum-check final evaluation mismatch")
    rho = transcript.squeeze_challenge()
    T = (vA + rho * vB + rho * rho % P * vC) % P
    final, r_y = sc.verify(sc.Evaluations, l, 2, T, transcript)
    eA, eB, eC = transcript.read_field_elements(3)
    e_w = transcript.read_field_element()
    weights = eq_xy(r_b)
    xbar = [sum(weights[i] * x[j] for i, x in enumerate(xs)) % P for j in range(p)]
    top = r_y[l - 1]
    z_ry = ((1 - top) * e_w + top * spa.public_eval(xbar, r_y[:l - 1])) % P
    if final != (eA + rho * eB + rho * rho % P * eC) * z_ry % P:
        raise spa.SpartanError("inner sum-check final evaluation mismatch")
    point = r_b + r_y[:l - 1]
    kzg.batch_verify(vp.trim(k + l - 1), k + l - 1, cw, [point], spa._w_evaluations(e_w), transcript)
    for i, (b, value) in enumerate(zip(blobs, (eA, eB, eC))):
        spa._spark_verify_midstream(vp, n, l, b, r_x + r_y, value, transcript, i == 2)
    if transcript.pos != len(transcript.stream):
        raise spa.SpartanError("trailing bytes in proof")


# ------------------------------------------------------------------ the named cases: (n, l, p, K')
CASES = {
    "pair": (1, 2, 1, 2),
    "four": (3, 3, 2, 4),
    "three": (3, 3, 2, 3),
    "eight": (5, 3, 2, 8),
    "tall": (2, 4, 3, 4),
    "full_public": (3, 3, 4, 2),
    "twice": (3, 3, 2, 2),
    "mid": (12, 10, 5, 5),
}
# `twice` cannot be proved, by a rule of the PCS and not of this argument: with the same assignment twice W does not depend
# on the instance coordinate, its quotient by that coordinate is zero, and the transcript refuses to write the identity
# (oracle/pyref/kzg.py open_).  The case stays, as a refusal: the words, and the bytes written before it
REFUSED = {"twice": "Invalid elliptic curve point encoding"}
SMALL = [c for c in CASES if max(CASES[c][0], CASES[c][1] + batch_vars(CASES[c][3]) - 1) <= 6]
# `four` and `three` draw from one seed: `three` is the first three instances of `four`, over the same key
_SEED_OF = {"three": "four"}
_INSTANCES = {}


def _rng(case, what):
    return random.Random(zlib.crc32(repr(("spartan_batch", case, what)).encode()))


def case_instance(case):
    """-> (instance, ws, xs): K' different satisfying assignments of one circuit (nova_ref.circuit); computed once per case"""
    if case not in _INSTANCES:
        n, l, p, count = CASES[case]
        seed = _SEED_OF.get(case, case)
        draw = CASES[seed][3] if case != "twice" else 1
        inst, assigns = nv.circuit(_rng(seed, "instance"), n, l, p, draw)
        if case == "twice":
            assigns = assigns * 2
        assigns = assigns[:count]
        _INSTANCES[case] = (inst, [w for w, _ in assigns], [x for _, x in assigns])
    return _INSTANCES[case]


# ------------------------------------------------------------------ forgeries: name -> the verifier's words
FORGERIES = {
    "bad_witness": "outer sum-check final evaluation mismatch",
    "bad_eval": "inner sum-check final evaluation mismatch",
    "bad_public": "Consistency failure at round 1",  # (the public inputs are absorbed: every challenge differs)
    "swapped_publics": "Consistency failure at round 1",
    "other_count": "Consistency failure at round 1",  # (K' is absorbed)
}


def forgery(name):
    """-> (case, ws, xs_proved, xs_verified, forge): on `four`'s instance (other_count: `three`'s, over the same key)"""
    inst, ws, xs = case_instance("four")
    l = CASES["four"][1]
    if name == "bad_witness":
        # an OUTPUT entry of the LAST instance's w: the row it closes fails, in the high instance lanes
        last = len(ws) - 1
        for y in range(len(ws[last]) - 1, -1, -1):
            w2 = list(ws[last])
            w2[y] = (w2[y] + 1) % P
            if spa.satisfied(inst, w2, xs[last], l) == 1:
                return "four", ws[:last] + [w2], xs, xs, "bad_witness"
        raise AssertionError("no witness entry fails exactly one row")
    if name == "bad_eval":
        return "four", ws, xs, xs, "bad_eval"
    if name == "bad_public":
        other = [list(x) for x in xs]
        other[2][1] = (other[2][1] + 1) % P
        return "four", ws, xs, other, None
    if name == "swapped_publics":
        assert xs[0] != xs[1]
        return "four", ws, xs, [xs[1], xs[0]] + xs[2:], None
    if name == "other_count":
        _, ws3, xs3 = case_instance("three")
        return "three", ws3, xs3, xs3 + [[0] * len(xs3[0])], None
    raise KeyError(name)
