"""Gemini over univariate KZG, and the batched univariate KZG opening under it.  TEST INFRASTRUCTURE ONLY (not a test file).

A big-int restatement, written from the reference's text, of
  UnivariateKzg::{commit, open, batch_open, verify, batch_verify}   pcs/univariate/kzg.rs:242-555
  Gemini::{commit, open, batch_open, verify, batch_verify}          pcs/multilinear/gemini.rs:56-211
  barycentric_weights / barycentric_interpolate                     util/arithmetic.rs:108-136
  UnivariatePolynomial::{new (leading zeros dropped), div_rem}      poly/univariate.rs
with the module interface oracle/pyref/lasso.py `prove(..., pcs=...)` and oracle/pyref/hyperplonk.py expect from
`zeromorph` (commit, batch_commit_and_write, batch_open, batch_verify on trimmed params).

Polynomial division here is schoolbook div_rem by the EXPANDED vanishing polynomial, as the reference's; the library
divides by the linear factors one after the other (and by X^2 - beta^2 in one stride-2 pass): the oracle does not share
that shortcut.  The verifier checks the pairing equation e(c, -[1]_2) e(pi, [s]_2) = 1 in its trapdoor form c == s * pi
(the library's host verifier uses the real pairing).

Two things the reference does that a reader may not expect, kept here:
  * a commitment that is the identity cannot be written to a transcript (util/transcript.rs:172-179, "Invalid elliptic
    curve point encoding"): an opening of one variable - its only quotient, fs[0] div (X^2 - beta^2), is zero - and an
    opening of the all-zero table end with that TranscriptError;
  * degrees are checked after leading zeros are dropped.
"""
from oracle.pyref.field import R_MOD as P
from oracle.pyref import curve, kzg, sum_check as sc, expression as ex, zeromorph
from oracle.pyref.field import batch_invert
from oracle.pyref.poly import eq_xy, eq_xy_eval

Evaluation = kzg.Evaluation
PcsError = kzg.PcsError
setup = zeromorph.setup          # UnivariateKzg::setup (kzg.rs:175-218), trapdoor explicit
commit_coeffs = zeromorph.commit_coeffs


class ProverParam:
    """UnivariateKzgProverParam (kzg.rs:68-88)"""

    def __init__(self, powers):
        self.powers = powers

    @property
    def degree(self):
        return len(self.powers) - 1


class VerifierParam:
    def __init__(self, s):
        self.s = s % P  # stands for (g1, g2, [s]_2)


def trim(param, poly_size):
    """kzg.rs:220-240"""
    if len(param.powers_g1) < poly_size:
        raise PcsError("Too large poly_size to trim to")
    return ProverParam(param.powers_g1[:poly_size]), VerifierParam(param.s)


# ------------------------------------------------------------------ UnivariatePolynomial
def _trunc(c):
    c = [v % P for v in c]
    while c and c[-1] == 0:
        c.pop()
    return c


def _degree(c):
    return max(len(_trunc(c)) - 1, 0)


def poly_eval(c, x):
    acc = 0
    for v in reversed(c):
        acc = (acc * x + v) % P
    return acc


def poly_add_scaled(acc, scalar, c):
    out = list(acc) + [0] * max(len(c) - len(acc), 0)
    for i, v in enumerate(c):
        out[i] = (out[i] + scalar * v) % P
    return out


def vanishing_poly(points):
    """UnivariatePolynomial::basis(points, 1) = prod (X - p)"""
    c = [1]
    for p in points:
        nxt = [0] * (len(c) + 1)
        for i, v in enumerate(c):
            nxt[i + 1] = (nxt[i + 1] + v) % P
            nxt[i] = (nxt[i] - p * v) % P
        c = nxt
    return c


def div_rem(f, d):
    """schoolbook long division (univariate.rs div_rem) -> (quotient, remainder), both truncated"""
    f, d = _trunc(f), _trunc(d)
    assert d
    if len(f) < len(d):
        return [], f
    rem, q = list(f), [0] * (len(f) - len(d) + 1)
    lead_inv = pow(d[-1], P - 2, P)
    for i in range(len(q) - 1, -1, -1):
        coef = rem[i + len(d) - 1] * lead_inv % P
        q[i] = coef
        if coef:
            for j, dv in enumerate(d):
                rem[i + j] = (rem[i + j] - coef * dv) % P
    return _trunc(q), _trunc(rem[:len(d) - 1])


# ------------------------------------------------------------------ UnivariateKzg
def ukzg_commit(pp, coeffs):
    """kzg.rs:242-252"""
    if pp.degree < _degree(coeffs):
        raise PcsError("Too large degree of poly to commit (param supports degree up to %d but got %d)"
                       % (pp.degree, _degree(coeffs)))
    return commit_coeffs(pp.powers, _trunc(coeffs))


def ukzg_open(pp, coeffs, point, transcript):
    """kzg.rs:264-299"""
    if pp.degree < _degree(coeffs):
        raise PcsError("Too large degree of poly to open (param supports degree up to %d but got %d)"
                       % (pp.degree, _degree(coeffs)))
    quotient, _ = div_rem(coeffs, [(-point) % P, 1])
    transcript.write_commitment(commit_coeffs(pp.powers, quotient))


def ukzg_verify(vp, comm, point, eval_, transcript):
    """kzg.rs:366-378: c = pi * point + comm - g1 * eval;  e(c, -g2) e(pi, [s]_2) == 1  <=>  c == s * pi"""
    pi = transcript.read_commitment()
    c = curve.add(curve.add(curve.mul(pi, point % P), comm), curve.neg(curve.mul(curve.G1_GEN, eval_ % P)))
    if c != curve.mul(pi, vp.s):
        raise PcsError("Invalid univariate KZG open")


class EvaluationSet:
    def __init__(self, polys, points, diffs, evals):
        self.polys, self.points, self.diffs, self.evals = polys, points, diffs, evals


def eval_sets(evals):
    """kzg.rs:454-512 -> (sets, superset as a sorted list)"""
    poly_shifts, superset = [], set()
    for ev in evals:
        for ps in poly_shifts:
            if ps[0] == ev.poly:
                if ev.point not in ps[1]:
                    ps[1].append(ev.point)
                    ps[2].append(ev.value)
                break
        else:
            poly_shifts.append((ev.poly, [ev.point], [ev.value]))
        superset.add(ev.point)
    sets = []
    for poly, points, values in poly_shifts:
        for st in sets:
            if set(st.points) == set(points):
                if poly not in st.polys:
                    st.polys.append(poly)
                    st.evals.append([values[points.index(p)] for p in st.points])
                break
        else:
            sets.append(EvaluationSet([poly], points, [p for p in sorted(superset) if p not in points], [values]))
    return sets, sorted(superset)


def vanishing_eval(points, z):
    acc = 1
    for p in points:
        acc = acc * (z - p) % P
    return acc


def set_scalars(sets, powers_of_gamma, points, z):
    """kzg.rs:514-533"""
    vde = [vanishing_eval([points[i] for i in st.diffs], z) for st in sets]
    normalizer = pow(vde[0], P - 2, P) if vde[0] else 1
    return [normalizer * v * g % P for v, g in zip(vde, powers_of_gamma)], normalizer


def comm_scalars(num_polys, sets, powers_of_beta, normalized_scalars):
    """kzg.rs:541-555"""
    scalars = [0] * num_polys
    for st, coeff in zip(sets, normalized_scalars):
        for poly, pb in zip(st.polys, powers_of_beta):
            scalars[poly] = coeff * pb % P
    return scalars


def barycentric_weights(points):
    w = []
    for j, pj in enumerate(points):
        acc = 1
        for i, pi in enumerate(points):
            if i != j:
                acc = acc * (pj - pi) % P
        w.append(acc)
    return batch_invert(w)


def barycentric_interpolate(weights, points, evals, x):
    coeffs = [c * w % P for c, w in zip(batch_invert([(x - p) % P for p in points]), weights)]
    s = sum(coeffs) % P
    if s == 0:
        raise ZeroDivisionError("barycentric_interpolate: x is one of the points")
    return sum(c * e for c, e in zip(coeffs, evals)) % P * pow(s, P - 2, P) % P


def _powers(x, n):
    out, p = [], 1
    for _ in range(n):
        out.append(p)
        p = p * x % P
    return out


def ukzg_batch_open(pp, polys, points, evals, transcript):
    """kzg.rs:301-354 (no sanity-check: the comm and eval handed to the final open are defaults)"""
    sets, superset = eval_sets(evals)
    beta = transcript.squeeze_challenge()
    gamma = transcript.squeeze_challenge()
    pob = _powers(beta, max(len(st.polys) for st in sets))
    pog = _powers(gamma, len(sets))
    fs, qs = [], []
    for st in sets:
        f = []
        for b, poly in zip(pob, st.polys):
            f = poly_add_scaled(f, b, polys[poly])
        q, _ = div_rem(f, vanishing_poly([points[i] for i in st.points]))
        fs.append(_trunc(f)), qs.append(q)
    q = []
    for g, q_s in zip(pog, qs):
        q = poly_add_scaled(q, g, q_s)
    q = _trunc(q)
    transcript.write_commitment(ukzg_commit(pp, q))
    z = transcript.squeeze_challenge()
    normalized, normalizer = set_scalars(sets, pog, points, z)
    q_scalar = (-vanishing_eval([points[i] for i in superset], z) * normalizer) % P
    f = []
    for s_, f_s in zip(normalized, fs):
        f = poly_add_scaled(f, s_, f_s)
    f = poly_add_scaled(f, q_scalar, q)
    ukzg_open(pp, f, z, transcript)


def ukzg_batch_verify(vp, comms, points, evals, transcript):
    """kzg.rs:380-419"""
    sets, superset = eval_sets(evals)
    beta = transcript.squeeze_challenge()
    gamma = transcript.squeeze_challenge()
    q_comm = transcript.read_commitment()
    z = transcript.squeeze_challenge()
    pob = _powers(beta, max(len(st.polys) for st in sets))
    pog = _powers(gamma, len(sets))
    normalized, normalizer = set_scalars(sets, pog, points, z)
    scalars = comm_scalars(len(comms), sets, pob, normalized)
    q_scalar = (-vanishing_eval([points[i] for i in superset], z) * normalizer) % P
    f = curve.msm(scalars + [q_scalar], list(comms) + [q_comm])
    r_evals = []
    for st in sets:
        pts = [points[i] for i in st.points]
        w = barycentric_weights(pts)
        r = [barycentric_interpolate(w, pts, e, z) for e in st.evals]
        r_evals.append(sum(b * v for b, v in zip(pob, r)) % P)
    eval_ = sum(a * b for a, b in zip(normalized, r_evals)) % P
    ukzg_verify(vp, f, z, eval_, transcript)


# ------------------------------------------------------------------ Gemini
def commit(pp, evals):
    """gemini.rs:56-66: the table is committed as a coefficient vector (same bytes as Zeromorph's commit)"""
    if pp.degree + 1 < len(evals):
        raise PcsError("Too large degree of poly to commit (param supports degree up to %d but got %d)"
                       % (pp.degree, len(evals)))
    return commit_coeffs(pp.powers, evals)


def batch_commit_and_write(pp, polys, transcript):
    comms = [commit(pp, p) for p in polys]
    transcript.write_commitments(comms)
    return comms


def gemini_folds(evals, point):
    """gemini.rs:100-108: fs[i][j] = fs[i-1][2j] + x_{i-1} (fs[i-1][2j+1] - fs[i-1][2j])"""
    fs = [[v % P for v in evals]]
    for x in point[:-1]:
        prev = fs[-1]
        fs.append([(prev[2 * j] + x * (prev[2 * j + 1] - prev[2 * j])) % P for j in range(len(prev) // 2)])
    return fs


def _squares(beta, n):
    out = [beta % P]
    while len(out) < n:
        out.append(out[-1] * out[-1] % P)
    return out[:n]


def _gemini_queries(n):
    return [(0, 0), (0, 1)] + [(i, i + 1) for i in range(1, n)]


def open_(pp, evals, point, eval_, transcript):
    """gemini.rs:78-138 (`eval_` is only read by the sanity-check feature)"""
    n = len(point)
    assert n >= 1 and len(evals) == 1 << n
    if pp.degree + 1 < len(evals):
        raise PcsError("Too large degree of poly to open (param supports degree up to %d but got %d)"
                       % (pp.degree, len(evals)))
    fs = gemini_folds(evals, point)
    transcript.write_commitments([ukzg_commit(pp, f) for f in fs[1:]])
    beta = transcript.squeeze_challenge()
    points = ([beta] + [(-v) % P for v in _squares(beta, n)])[:n + 1]
    evs = [Evaluation(i, p, poly_eval(fs[i], points[p])) for i, p in _gemini_queries(n)]
    transcript.write_field_elements([e.value for e in evs[1:]])
    ukzg_batch_open(pp, fs, points, evs, transcript)


def verify(vp, comm, point, eval_, transcript):
    """gemini.rs:165-198"""
    n = len(point)
    comms = [comm] + transcript.read_commitments(n - 1)
    beta = transcript.squeeze_challenge()
    sq = _squares(beta, n)
    evs = transcript.read_field_elements(n)
    e0 = eval_ % P
    for e_neg, s, x in reversed(list(zip(evs, sq, point))):
        den = ((1 - x) * s + x) % P
        if den == 0:
            raise ZeroDivisionError("gemini verify: zero denominator")
        e0 = (2 * s * e0 - ((1 - x) * s - x) * e_neg) % P * pow(den, P - 2, P) % P
    evals = [Evaluation(i, p, v) for (i, p), v in zip(_gemini_queries(n), [e0] + evs)]
    points = [beta % P] + [(-v) % P for v in sq]
    ukzg_batch_verify(vp, comms, points, evals, transcript)


def batch_open(pp, num_vars, polys, points, evals, transcript):
    """additive::batch_open (pcs/multilinear.rs:134-235) with Pcs = Gemini; g_prime_eval is passed as zero"""
    ell = (len(evals) - 1).bit_length() if len(evals) > 1 else 0
    t = transcript.squeeze_challenges(ell)
    eq_xt = eq_xy(t) if ell else []
    if not eq_xt:
        raise PcsError("batch_open needs >= 2 evaluations")
    merged = kzg._merged(polys, points, evals, eq_xt)
    expression = ex.sum_exprs(ex.EqXY(j) * ex.Poly(j) * 1 for j in range(len(points)))
    vp = sc.VirtualPolynomial(expression, merged, [], points)
    tilde_gs_sum = sum(ev.value * w for ev, w in zip(evals, eq_xt)) % P
    challenges, _ = sc.prove(sc.CoefficientsProver, num_vars, vp, tilde_gs_sum, transcript)
    g_prime = [0] * (1 << num_vars)
    for m, pt in zip(merged, points):
        w = eq_xy_eval(challenges, pt)
        g_prime = [(a + w * v) % P for a, v in zip(g_prime, m)]
    open_(pp, g_prime, challenges, 0, transcript)


def batch_verify(vp, num_vars, comms, points, evals, transcript):
    """additive::batch_verify (pcs/multilinear.rs:237-276) with Pcs = Gemini"""
    ell = (len(evals) - 1).bit_length() if len(evals) > 1 else 0
    t = transcript.squeeze_challenges(ell)
    eq_xt = eq_xy(t)
    tilde_gs_sum = sum(ev.value * w for ev, w in zip(evals, eq_xt)) % P
    g_prime_eval, challenges = sc.verify(sc.Coefficients, num_vars, 2, tilde_gs_sum, transcript)
    eq_evals = [eq_xy_eval(challenges, pt) for pt in points]
    scalars = [eq_evals[ev.point] * w % P for ev, w in zip(evals, eq_xt)]
    g_prime_comm = curve.msm(scalars, [comms[ev.poly] for ev in evals])
    verify(vp, g_prime_comm, challenges, g_prime_eval, transcript)
