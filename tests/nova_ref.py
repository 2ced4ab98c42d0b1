"""TEST INFRASTRUCTURE ONLY: Nova folding (Kothapalli, Setty, Tzialla, CRYPTO 2022) for the R1CS keys of tests/spartan_ref.py,
and the relaxed form of Spartan that closes a chain of folds - on top of oracle/pyref, tests/spark_ref.py and
tests/spartan_ref.py, all unchanged.  This file is the specification of lh_nova_instance / lh_nova_fold / lh_nova_fold_verify /
lh_spartan_prove_relaxed / lh_spartan_verify_relaxed: the HIP prover reproduces these bytes.

Statement: a relaxed instance over a key (n, l) with p public inputs is (C_W, C_E, x): C_W the commitment of w over l - 1
variables, C_E the one of the error vector E over l variables, x the p public inputs with u = x[0].  Its witness is (w, E);
the relation is (Az)[i] (Bz)[i] = u (Cz)[i] + E[i] for every row, z = (w, x, 0) as in spartan_ref.  A fresh instance has E = 0
(E is then given as None), C_E the identity and x[0] = 1.

The instance blob is a transcript's stream of its own: o_lasso.write_commitments of [C_W, C_E] (the mask element, the
non-identity points), then write_field_elements of x.

Fold of (U1, W1) and (U2, W2), either of them relaxed (transcript order == proof layout):

 0.     z1, z2; A z1 .. C z2; T = Az1 Bz2 + Az2 Bz1 - u1 Cz2 - u2 Cz1; the rows at which an input fails its own relation are
        counted: an input that does is refused BEFORE step 1 (input 1 first)
 1. C   n, l, p; per matrix of the key its commitment's mask and its points (as spartan_ref._header); per instance its mask
        (common_field_element), its points (common_commitment), its x
 2. W   ONE write_commitments block of T (l variables)
 3. S   r
 4.     w = w1 + r w2, E = E1 + r T + r^2 E2, x = x1 + r x2, C_W = C_W1 + r C_W2, C_E = C_E1 + r C_T + r^2 C_E2

The verifier of a fold does 1, reads 2, does 3 and the instance half of 4: no pairing.

Relaxed Spartan: spartan_ref's schedule with four differences.  The header absorbs n, l, p and the key, then the instance as
in step 1 above (C_W is not written into the proof).  The outer expression is EqXY(0) (Poly(0) Poly(1) - u Poly(2) - Poly(3))
over [Az, Bz, Cz, E], claim 0; vA, vB, vC, vE are written.  After the opening of w, E is opened at r_x over l variables with the
same doubled-evaluation list - unless the instance's mask says C_E is the identity: no opening then, and the verifier
requires vE = 0.  The outer final claim is eq(tau, r_x) (vA vB - u vC - vE).
"""
import random
import zlib

import spark_ref as spr
import spartan_ref as spa
from oracle.pyref import curve
from oracle.pyref import expression as ex
from oracle.pyref import kzg
from oracle.pyref import lasso as o_lasso
from oracle.pyref import sum_check as sc
from oracle.pyref.field import R_MOD as P
from oracle.pyref.poly import eq_xy, eq_xy_eval, evaluate
from oracle.pyref.transcript import Keccak256Transcript, TranscriptError


class NovaError(Exception):
    pass


class Instance:
    """(C_W, C_E, x): commitments are points or None for the identity"""

    def __init__(self, cw, ce, x):
        self.cw, self.ce, self.x = cw, ce, [v % P for v in x]

    @property
    def blob(self):
        t = Keccak256Transcript()
        o_lasso.write_commitments(t, [self.cw, self.ce])
        t.write_field_elements(self.x)
        return t.into_proof()


def read_instance(blob, p):
    """-> Instance; the blob is a transcript's stream of its own"""
    t = Keccak256Transcript(blob)
    try:
        cw, ce = o_lasso.read_commitments(t, 2)
        x = t.read_field_elements(p)
    except (TranscriptError, o_lasso.LassoError) as e:
        raise NovaError("malformed instance: %s" % e)
    if t.pos != len(t.stream):
        raise NovaError("malformed instance: wrong length")
    return Instance(cw, ce, x)


def fresh(pp, key, w, x):
    """the instance of a plain satisfying assignment (x[0] = 1): C_E the identity"""
    l = key.l
    spa._shape(key.n, l, len(x))
    if x[0] % P != 1:
        raise NovaError("a fresh instance has x[0] = 1")
    mats = [(m.dims[0], m.dims[1], m.val) for m in key.mats]
    z = spa.assignment(l, w, x)
    Mz = [spa.spmv(row, col, val, z, 1 << l) for row, col, val in mats]
    bad = sum(1 for a, b, c in zip(*Mz) if (a * b - c) % P)
    if bad:
        raise NovaError("the witness does not satisfy %d of the 2^%d constraints" % (bad, l))
    return Instance(kzg.commit(pp.trim(l - 1), [v % P for v in w]), None, x)


def products(key, w, x):
    l = key.l
    z = spa.assignment(l, w, x)
    return [spa.spmv(m.dims[0], m.dims[1], m.val, z, 1 << l) for m in key.mats]


def unsatisfied(Mz, u, E):
    """the rows at which Az Bz != u Cz + E (E None: zero)"""
    return sum(1 for i, (a, b, c) in enumerate(zip(*Mz)) if (a * b - u * c - (E[i] if E is not None else 0)) % P)


def relaxed_satisfied(instance, w, E, x, l):
    """from the dense matrices: independent of the sparse path -> the number of rows that fail the relaxed relation"""
    M = 1 << l
    z = spa.assignment(l, w, x)
    prods = []
    for row, col, val in instance:
        dense = [[0] * M for _ in range(M)]
        for r, c, v in zip(row, col, val):
            dense[r][c] = (dense[r][c] + v) % P
        prods.append([sum(a * b for a, b in zip(dense[i], z)) % P for i in range(M)])
    return unsatisfied(prods, x[0] % P, E)


def _key_header(transcript, n, l, p, key_comms):
    transcript.common_field_elements([n, l, p])
    for comms in key_comms:
        transcript.common_field_element(sum(1 << i for i, cm in enumerate(comms) if cm is None))
        for cm in comms:
            if cm is not None:
                transcript.common_commitment(cm)


def _absorb_instance(transcript, U):
    comms = [U.cw, U.ce]
    transcript.common_field_element(sum(1 << i for i, cm in enumerate(comms) if cm is None))
    for cm in comms:
        if cm is not None:
            transcript.common_commitment(cm)
    transcript.common_field_elements(U.x)


def _fold_instances(U1, U2, ct, r):
    r2 = r * r % P
    return Instance(curve.add(U1.cw, curve.mul(U2.cw, r)),
                    curve.add(curve.add(U1.ce, curve.mul(ct, r)), curve.mul(U2.ce, r2)),
                    [(a + r * b) % P for a, b in zip(U1.x, U2.x)])


def cross_term(key, U1, W1, U2, W2):
    """step 0 -> T; an input that fails its own relation is refused, input 1 first"""
    (w1, E1), (w2, E2) = W1, W2
    u1, u2 = U1.x[0], U2.x[0]
    Mz1, Mz2 = products(key, w1, U1.x), products(key, w2, U2.x)
    for k, (Mz, u, E) in enumerate(((Mz1, u1, E1), (Mz2, u2, E2))):
        bad = unsatisfied(Mz, u, E)
        if bad:
            raise NovaError("input %d does not satisfy %d of the 2^%d constraints" % (k + 1, bad, key.l))
    return [(a1 * b2 + a2 * b1 - u1 * c2 - u2 * c1) % P for (a1, b1, c1), (a2, b2, c2) in zip(zip(*Mz1), zip(*Mz2))]


def fold_witness(W1, W2, T, r):
    """step 4's witness half"""
    (w1, E1), (w2, E2) = W1, W2
    r2 = r * r % P
    w = [(a + r * b) % P for a, b in zip(w1, w2)]
    E = [((E1[i] if E1 is not None else 0) + r * T[i] + (r2 * E2[i] if E2 is not None else 0)) % P for i in range(len(T))]
    return w, E


def fold(pp, key, U1, W1, U2, W2, transcript, forge=None):
    """W = (w, E) with E None for zero.  Appends the proof (the T block) to `transcript` -> (U, (w, E)).
    forge (tests only): "bad_T" commits to and folds a T whose entry 0 is off by one."""
    n, l, p = key.n, key.l, len(U1.x)
    spa._shape(n, l, p)
    if len(U2.x) != p:
        raise NovaError("the two instances have different numbers of public inputs")
    T = cross_term(key, U1, W1, U2, W2)
    if forge == "bad_T":
        T[0] = (T[0] + 1) % P
    _key_header(transcript, n, l, p, [m.comms for m in key.mats])
    _absorb_instance(transcript, U1)
    _absorb_instance(transcript, U2)
    ct = kzg.commit(pp.trim(l), T)
    o_lasso.write_commitments(transcript, [ct])
    r = transcript.squeeze_challenge()
    return _fold_instances(U1, U2, ct, r), fold_witness(W1, W2, T, r)


def fold_verify(n, l, p, key_blob, blob1, blob2, transcript, challenge=None):
    """-> the folded instance's blob (challenge: a list that takes r).  Raises NovaError on blobs or a proof that cannot be read."""
    spa._shape(n, l, p)
    try:
        key_comms = [spr.read_commitment_blob(b, 2)[1] for b in spa.split_key(key_blob)]
    except (spa.SpartanError, spr.SparkError) as e:
        raise NovaError("malformed key: %s" % e)
    U1, U2 = read_instance(blob1, p), read_instance(blob2, p)
    _key_header(transcript, n, l, p, key_comms)
    _absorb_instance(transcript, U1)
    _absorb_instance(transcript, U2)
    try:
        ct, = o_lasso.read_commitments(transcript, 1)
    except (TranscriptError, o_lasso.LassoError) as e:
        raise NovaError(str(e))
    r = transcript.squeeze_challenge()
    if transcript.pos != len(transcript.stream):
        raise NovaError("trailing bytes in proof")
    if challenge is not None:
        challenge.append(r)
    return _fold_instances(U1, U2, ct, r).blob


# ------------------------------------------------------------------ relaxed Spartan
def _outer_expression(u):
    return ex.EqXY(0) * (ex.Poly(0) * ex.Poly(1) - ex.Poly(2) * u - ex.Poly(3))


def prove_relaxed(pp, key, U, W, transcript, forge=None):
    """Appends the proof to `transcript`.  forge (tests only): "unsatisfied" goes on with a witness that fails the relaxed
    relation; "bad_vE" writes vE + 1."""
    n, l, p = key.n, key.l, len(U.x)
    spa._shape(n, l, p)
    M = 1 << l
    w, E = W
    w = [v % P for v in w]
    u = U.x[0]
    if (E is None) != (U.ce is None) and not (E is not None and not any(E)):
        raise NovaError("E and the instance's C_E do not go together")
    z = spa.assignment(l, w, U.x)
    mats = [(m.dims[0], m.dims[1], m.val) for m in key.mats]
    Mz = [spa.spmv(row, col, val, z, M) for row, col, val in mats]
    bad = unsatisfied(Mz, u, E)
    if bad and forge != "unsatisfied":
        raise spa.SpartanError("the witness does not satisfy %d of the 2^%d constraints" % (bad, l))
    Ev = [v % P for v in E] if E is not None else [0] * M
    _key_header(transcript, n, l, p, [m.comms for m in key.mats])
    _absorb_instance(transcript, U)
    tau = transcript.squeeze_challenges(l)
    r_x, at_rx = sc.prove(sc.EvaluationsProver, l, sc.VirtualPolynomial(_outer_expression(u), Mz + [Ev], [], [tau]), 0, transcript)
    v = list(at_rx[:4])
    if forge == "bad_vE":
        v[3] = (v[3] + 1) % P
    transcript.write_field_elements(v)
    rho = transcript.squeeze_challenge()
    T = (at_rx[0] + rho * at_rx[1] + rho * rho % P * at_rx[2]) % P
    eq_rx = eq_xy(r_x)
    Mc = [spa.spmv(col, row, val, eq_rx, M) for row, col, val in mats]
    r_y, at_ry = sc.prove(sc.EvaluationsProver, l, sc.VirtualPolynomial(spa._inner_expression(rho), Mc + [z], [], []), T, transcript)
    transcript.write_field_elements(at_ry[:3])
    e_w = evaluate(w, r_y[:l - 1])
    transcript.write_field_element(e_w)
    kzg.batch_open(pp.trim(l - 1), l - 1, [w], [r_y[:l - 1]], spa._w_evaluations(e_w), transcript)
    if U.ce is not None:
        kzg.batch_open(pp.trim(l), l, [Ev], [r_x], spa._w_evaluations(v[3]), transcript)
    for m, want in zip(key.mats, at_ry[:3]):
        got = spr.open_(pp, m, r_x + r_y, transcript)
        assert got == want


def verify_relaxed(vp, n, l, p, key_blob, blob, transcript):
    """Raises SpartanError on any proof that does not verify (a piece's own refusal keeps its words)."""
    try:
        _verify_relaxed(vp, n, l, p, key_blob, blob, transcript)
    except (sc.SumCheckError, kzg.PcsError, o_lasso.LassoError, TranscriptError) as e:
        raise spa.SpartanError(str(e))
    except NovaError as e:
        raise spa.SpartanError(str(e))


def _verify_relaxed(vp, n, l, p, key_blob, blob, transcript):
    spa._shape(n, l, p)
    blobs = spa.split_key(key_blob)
    try:
        comm_lists = [spr.read_commitment_blob(b, 2)[1] for b in blobs]
    except spr.SparkError as e:
        raise spa.SpartanError("malformed key: %s" % e)
    U = read_instance(blob, p)
    x, u = U.x, U.x[0]
    _key_header(transcript, n, l, p, comm_lists)
    _absorb_instance(transcript, U)
    tau = transcript.squeeze_challenges(l)
    final, r_x = sc.verify(sc.Evaluations, l, 3, 0, transcript)
    vA, vB, vC, vE = transcript.read_field_elements(4)
    if U.ce is None and vE:
        raise spa.SpartanError("vE is not zero though C_E is the identity")
    if final != eq_xy_eval(tau, r_x) * (vA * vB - u * vC - vE) % P:
        raise spa.SpartanError("outer sum-check final evaluation mismatch")
    rho = transcript.squeeze_challenge()
    T = (vA + rho * vB + rho * rho % P * vC) % P
    final, r_y = sc.verify(sc.Evaluations, l, 2, T, transcript)
    eA, eB, eC = transcript.read_field_elements(3)
    e_w = transcript.read_field_element()
    top = r_y[l - 1]
    z_ry = ((1 - top) * e_w + top * spa.public_eval(x, r_y[:l - 1])) % P
    if final != (eA + rho * eB + rho * rho % P * eC) * z_ry % P:
        raise spa.SpartanError("inner sum-check final evaluation mismatch")
    kzg.batch_verify(vp.trim(l - 1), l - 1, [U.cw], [r_y[:l - 1]], spa._w_evaluations(e_w), transcript)
    if U.ce is not None:
        kzg.batch_verify(vp.trim(l), l, [U.ce], [r_x], spa._w_evaluations(vE), transcript)
    for i, (b, value) in enumerate(zip(blobs, (eA, eB, eC))):
        spa._spark_verify_midstream(vp, n, l, b, r_x + r_y, value, transcript, i == 2)
    if transcript.pos != len(transcript.stream):
        raise spa.SpartanError("trailing bytes in proof")


# ------------------------------------------------------------------ the named cases: (n, l, p)
CASES = {
    "tiny": (1, 2, 1),
    "chain": (3, 3, 2),
    "two_relaxed": (3, 3, 2),
    "self_fold": (3, 3, 1),
    "fresh_relaxed": (3, 3, 2),
    "tall": (2, 4, 3),
    "full_public": (3, 3, 4),
    "mid": (12, 10, 5),
}
SMALL = [k for k in CASES if max(CASES[k][:2]) <= 6]
# the fresh assignments a case draws
ASSIGNMENTS = {"tiny": 2, "chain": 4, "two_relaxed": 4, "self_fold": 1, "fresh_relaxed": 1, "tall": 2, "full_public": 2, "mid": 3}


def _rng(case, what):
    return random.Random(zlib.crc32(repr(("nova", case, what)).encode()))


def circuit(rng, n, l, p, count):
    """-> (instance, [(w, x), ..]): an instance that `count` different assignments satisfy.  A and B are what
    spartan_ref.satisfiable draws over the INPUT columns - the lower half of w and x -, their rows folded onto the first
    2^(l-2); row i of C is the one entry 1 at the OUTPUT column 2^(l-2) + i of w: w's upper half is (Az)[i] (Bz)[i], whatever
    the inputs are.  (satisfiable's own C is closed over one assignment: two assignments that both satisfy it have the same
    Az, Bz, Cz, and their cross term is identically zero.)"""
    N, M, half = 1 << n, 1 << l, 1 << (l - 1)
    outs = half // 2
    inputs = list(range(outs)) + [half + i for i in range(p)]
    (A, B, _), _, _ = spa.satisfiable(rng, n, l, p, a_cols=inputs)
    A, B = ([r % outs for r in A[0]], A[1], A[2]), ([r % outs for r in B[0]], B[1], B[2])
    rows = sorted(set(A[0]))
    pad = [0] * (N - len(rows))
    Cm = (rows + pad, [outs + i for i in rows] + pad, [1] * len(rows) + pad)
    assigns = []
    for _ in range(count):
        x = [1] + [rng.randrange(P) for _ in range(p - 1)]
        w = [rng.randrange(P) for _ in range(outs)] + [0] * outs
        z = spa.assignment(l, w, x)
        Az, Bz = spa.spmv(A[0], A[1], A[2], z, M), spa.spmv(B[0], B[1], B[2], z, M)
        for i in range(outs):
            w[outs + i] = Az[i] * Bz[i] % P
        assigns.append((w, x))
    return [A, B, Cm], assigns


_INSTANCES = {}


def case_instance(case):
    """-> (instance, [(w, x), ..]); computed once per case"""
    if case not in _INSTANCES:
        n, l, p = CASES[case]
        _INSTANCES[case] = circuit(_rng(case, "instance"), n, l, p, ASSIGNMENTS[case])
    return _INSTANCES[case]


# The schedule of a case: a list of steps over numbered slots.  ("fresh", k): slot <- the fresh instance of assignment k;
# ("fold", a, b): slot <- the fold of slots a and b, with E2 None when b is fresh; ("prove", a): the relaxed proof of slot a.
SCHEDULES = {
    "tiny": [("fresh", 0), ("fresh", 1), ("fold", 0, 1), ("prove", 2)],
    "chain": [("fresh", 0), ("fresh", 1), ("fresh", 2), ("fresh", 3), ("fold", 0, 1), ("fold", 4, 2), ("fold", 5, 3), ("prove", 6)],
    "two_relaxed": [("fresh", 0), ("fresh", 1), ("fresh", 2), ("fresh", 3), ("fold", 0, 1), ("fold", 2, 3), ("fold", 4, 5),
                    ("prove", 6)],
    "self_fold": [("fresh", 0), ("fold", 0, 0), ("prove", 1)],
    "fresh_relaxed": [("fresh", 0), ("prove", 0)],
    "tall": [("fresh", 0), ("fresh", 1), ("fold", 0, 1), ("prove", 2)],
    "full_public": [("fresh", 0), ("fresh", 1), ("fold", 0, 1), ("prove", 2)],
    "mid": [("fresh", 0), ("fresh", 1), ("fresh", 2), ("fold", 0, 1), ("fold", 3, 2), ("prove", 4)],
}


def run(pp, key, case, schedule=None, forge=None):
    """-> (slots, records): slots[i] = (Instance, (w, E)); records: per step a dict - "fresh": blob; "fold": a, b, proof,
    blob; "prove": a, proof.  forge "bad_T" damages the LAST fold, "bad_vE" the proof."""
    _, assigns = case_instance(case)
    steps = SCHEDULES[case] if schedule is None else schedule
    last_fold = max([i for i, s in enumerate(steps) if s[0] == "fold"], default=-1)
    slots, records = [], []
    for i, step in enumerate(steps):
        if step[0] == "fresh":
            w, x = assigns[step[1]]
            U = fresh(pp, key, w, x)
            slots.append((U, (w, None)))
            records.append({"step": "fresh", "blob": U.blob})
        elif step[0] == "fold":
            (U1, W1), (U2, W2) = slots[step[1]], slots[step[2]]
            t = Keccak256Transcript()
            U, W = fold(pp, key, U1, W1, U2, W2, t, forge="bad_T" if forge == "bad_T" and i == last_fold else None)
            slots.append((U, W))
            records.append({"step": "fold", "a": step[1], "b": step[2], "proof": t.into_proof(), "blob": U.blob})
        else:
            U, W = slots[step[1]]
            t = Keccak256Transcript()
            prove_relaxed(pp, key, U, W, t, forge={"bad_T": "unsatisfied", "bad_vE": "bad_vE"}.get(forge))
            records.append({"step": "prove", "a": step[1], "proof": t.into_proof()})
    return slots, records


# ------------------------------------------------------------------ forgeries: name -> the relaxed verifier's words
FORGERIES = {
    "bad_T": "outer sum-check final evaluation mismatch",
    "bad_vE": "outer sum-check final evaluation mismatch",
    # the instance the fold verifier returns for another U2 is absorbed by the relaxed verifier's header: every challenge
    # differs, round 0 still claims 0
    "other_input": "Consistency failure at round 1",
}
FORGERY_CASE = "chain"
