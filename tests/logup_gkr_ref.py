"""TEST INFRASTRUCTURE ONLY: LogUp-GKR - a stand-alone lookup argument for unstructured tables, looked up by value - on
top of oracle/pyref (gkr.prove_fractional_sum_check, kzg, lasso.write_commitments), in the style of tests/lasso_batch_ref.py.
This file is the specification of lh_logup_gkr_prove / lh_logup_gkr_verify: the HIP prover reproduces these proof bytes.

Statement: L lookups; lookup k has w_k input columns f_kj of 2^n field elements and a PUBLIC table of w_k columns t_kj of
2^l field elements; every input row equals some table row.  nv = max(n, l).  The table is part of the statement (like the
entries of a registered subtable): it is not absorbed into the transcript.

Protocol (transcript order == proof layout):

 0. C   L, n, l, w_0 .. w_{L-1}
 1. W   write_commitments of all input columns, lookup-major, each zero-padded to nv (one identity mask, then the points)
 2. S   beta;  cf_k = sum_j beta^j f_kj,  ct_k = sum_j beta^j t_kj  (squeezed for w = 1 too)
 3.     m_k over the 2^l table rows by hyperplonk.lookup_m_poly's rule (among equal rows the LAST index takes every count; an
        input that is not in the table: InvalidSnark "Invalid lookup input");  W  write_commitments of m_k padded to nv
 4. S   gamma
 5.     gkr.prove_fractional_sum_check over the L input fractions  1 / (gamma + cf_k), n variables, roots written -> x_n
 6.     gkr.prove_fractional_sum_check over the L table fractions  -m_k / (gamma + ct_k), l variables, roots written -> x_l
 7. W   f_kj(x_n) lookup-major, then m_k(x_l)
 8.     ONE batch_open over nv variables: polys = inputs then m's (commitment order), points x_n, x_l zero-padded,
        evaluations in the order of step 7

The verifier mirrors this; per lookup it checks Q_f != 0, Q_t != 0, P_f Q_t + P_t Q_f = 0 on the roots, the final claims
(input side p = 1, q = gamma + sum_j beta^j f_kj(x_n); table side p = -m_k(x_l), q = gamma + sum_j beta^j t~_kj(x_l) with
the table's multilinear extension evaluated on the host), batch_verify, and that no byte is left.
"""
import random
import zlib

from oracle.pyref import expression as ex
from oracle.pyref import gkr, kzg
from oracle.pyref import lasso as o_lasso
from oracle.pyref import sum_check as sc
from oracle.pyref.field import R_MOD as P
from oracle.pyref.poly import evaluate, eq_xy_eval

MAX_LOOKUPS = 8
MAX_WIDTH = 8
MAX_TABLE_VARS = 24
_R = (1 << 256) % P
_R_INV = pow(_R, -1, P)


class LogupError(Exception):
    pass


def _shape(widths, n, l):
    if not 1 <= len(widths) <= MAX_LOOKUPS:
        raise LogupError("1 to %d lookups" % MAX_LOOKUPS)
    if any(not 1 <= w <= MAX_WIDTH for w in widths):
        raise LogupError("width 1 to %d" % MAX_WIDTH)
    if not (1 <= n < 31 and 1 <= l <= MAX_TABLE_VARS):
        raise LogupError("num_vars / table_vars out of range")
    return max(n, l)


def compress(cols, beta):
    out, power = [0] * len(cols[0]), 1
    for col in cols:
        out = [(o + power * v) % P for o, v in zip(out, col)]
        power = power * beta % P
    return out


def multiplicities(cf, ct):
    """hyperplonk.lookup_m_poly with a table of its own size"""
    index = {}
    for i, t in enumerate(ct):
        index[t] = i
    m = [0] * len(ct)
    for v in cf:
        if v not in index:
            raise LogupError("Invalid lookup input")
        m[index[v]] += 1
    return m


def prove(pp, lookups, transcript, forge=None):
    """lookups: [(inputs, table)], inputs = w columns of 2^n ints, table = w columns of 2^l ints.
    forge (tests only): called with the honest-rule multiplicities' inputs (k, cf, ct), returns m_k - a cheating prover."""
    widths = [len(f) for f, _ in lookups]
    N, M = len(lookups[0][0][0]), len(lookups[0][1][0])
    n, l = N.bit_length() - 1, M.bit_length() - 1
    assert N == 1 << n and M == 1 << l
    assert all(len(f) == len(t) and all(len(c) == N for c in f) and all(len(c) == M for c in t) for f, t in lookups)
    nv = _shape(widths, n, l)
    L = len(lookups)
    transcript.common_field_elements([L, n, l] + widths)
    pp_nv = pp.trim(nv)
    polys = [o_lasso._pad(c, nv) for f, _ in lookups for c in f]
    o_lasso.write_commitments(transcript, [kzg.commit(pp_nv, p) for p in polys])
    beta = transcript.squeeze_challenge()
    cfs = [compress(f, beta) for f, _ in lookups]
    cts = [compress(t, beta) for _, t in lookups]
    ms = [forge(k, cf, ct) if forge else multiplicities(cf, ct) for k, (cf, ct) in enumerate(zip(cfs, cts))]
    m_polys = [o_lasso._pad(m, nv) for m in ms]
    o_lasso.write_commitments(transcript, [kzg.commit(pp_nv, p) for p in m_polys])
    polys += m_polys
    gamma = transcript.squeeze_challenge()
    none = [None] * L
    _, _, x_n = gkr.prove_fractional_sum_check(none, none, [[1] * N] * L, [[(gamma + v) % P for v in cf] for cf in cfs],
                                               transcript)
    _, _, x_l = gkr.prove_fractional_sum_check(none, none, [[-c % P for c in m] for m in ms],
                                               [[(gamma + v) % P for v in ct] for ct in cts], transcript)
    f_e = [evaluate(c, x_n) for f, _ in lookups for c in f]
    m_e = [evaluate(m, x_l) for m in ms]
    transcript.write_field_elements(f_e + m_e)
    evals = [kzg.Evaluation(i, 0, v) for i, v in enumerate(f_e)] + \
            [kzg.Evaluation(len(f_e) + k, 1, v) for k, v in enumerate(m_e)]
    points = [o_lasso._pad_point(x_n, nv), o_lasso._pad_point(x_l, nv)]
    kzg.batch_open(pp_nv, nv, polys, points, evals, transcript)
    return transcript


def verify_fractional_sum_check(num_vars, B, transcript):
    """gkr.verify_fractional_sum_check (fractional_sum_check.rs:193-270) with every root read, restated so that the roots
    are returned: -> (p_0s, q_0s, p_xs, q_xs, x)"""
    p_0s = transcript.read_field_elements(B)
    q_0s = transcript.read_field_elements(B)
    claimed_p, claimed_q = list(p_0s), list(q_0s)
    expression = gkr.frac_sum_check_expression(B)
    y = []
    for nv in range(num_vars):
        if nv == 0:
            evals = transcript.read_field_elements(4 * B)
            for b in range(B):
                p_l, p_r, q_l, q_r = evals[4 * b:4 * b + 4]
                if claimed_p[b] != (p_l * q_r + p_r * q_l) % P or claimed_q[b] != q_l * q_r % P:
                    raise gkr.GkrError("Unmatched between sum_check output and query evaluation")
            x = []
        else:
            gamma = transcript.squeeze_challenge()
            claim = gkr._frac_claim(claimed_p, claimed_q, gamma)
            x_eval, x = sc.verify(sc.Evaluations, nv, ex.degree(expression), claim, transcript)
            evals = transcript.read_field_elements(4 * B)
            if x_eval != ex.evaluate_fe(expression, [eq_xy_eval(x, y)], evals, [gamma]):
                raise gkr.GkrError("Unmatched between sum_check output and query evaluation")
        mu = transcript.squeeze_challenge()
        claimed_p, claimed_q = gkr._frac_down(evals, mu)
        y = x + [mu]
    return p_0s, q_0s, claimed_p, claimed_q, y


def verify(vp, tables, n, transcript):
    """tables: per lookup its w columns of 2^l ints.  Raises on any proof that does not verify."""
    widths = [len(t) for t in tables]
    M = len(tables[0][0])
    l = M.bit_length() - 1
    assert M == 1 << l and all(len(c) == M for t in tables for c in t)
    nv = _shape(widths, n, l)
    L = len(tables)
    transcript.common_field_elements([L, n, l] + widths)
    comms = o_lasso.read_commitments(transcript, sum(widths))
    beta = transcript.squeeze_challenge()
    comms += o_lasso.read_commitments(transcript, L)
    gamma = transcript.squeeze_challenge()
    pf, qf, pf_x, qf_x, x_n = verify_fractional_sum_check(n, L, transcript)
    pt, qt, pt_x, qt_x, x_l = verify_fractional_sum_check(l, L, transcript)
    for k in range(L):
        if qf[k] == 0 or qt[k] == 0 or (pf[k] * qt[k] + pt[k] * qf[k]) % P:
            raise LogupError("lookup %d: the fractions do not sum to zero" % k)
    f_e = transcript.read_field_elements(sum(widths))
    m_e = transcript.read_field_elements(L)
    at = 0
    for k, w in enumerate(widths):
        q_in, q_tab, power = gamma, gamma, 1
        for j in range(w):
            q_in = (q_in + power * f_e[at + j]) % P
            q_tab = (q_tab + power * evaluate(tables[k][j], x_l)) % P
            power = power * beta % P
        at += w
        if [pf_x[k], qf_x[k], pt_x[k], qt_x[k]] != [1, q_in, -m_e[k] % P, q_tab]:
            raise LogupError("lookup %d: leaf claim mismatch" % k)
    evals = [kzg.Evaluation(i, 0, v) for i, v in enumerate(f_e)] + \
            [kzg.Evaluation(len(f_e) + k, 1, v) for k, v in enumerate(m_e)]
    points = [o_lasso._pad_point(x_n, nv), o_lasso._pad_point(x_l, nv)]
    kzg.batch_verify(vp.trim(nv), nv, comms, points, evals, transcript)
    if transcript.pos != len(transcript.stream):
        raise LogupError("trailing bytes in proof")


# ------------------------------------------------------------------ the named cases: (n, l, widths)
CASES = {
    "one_var": (1, 1, [1]),
    "small_table": (5, 3, [3, 1]),
    "big_table": (2, 4, [2]),
    "square": (6, 6, [1, 2]),
    "dup": (4, 3, [1]),
    "zeros": (4, 3, [1]),
    "one_row": (4, 3, [2]),
    "collide": (4, 3, [1]),
    "mid": (13, 9, [2, 1]),
}
SMALL = [c for c in CASES if max(CASES[c][:2]) <= 6]  # the cases the golden SRS of six variables covers
MID_SRS_SEED = 0x10C0B


def mid_ss():
    """the seeded secrets of the 14-variable SRS of `mid`"""
    rng = random.Random(MID_SRS_SEED)
    return [rng.randrange(1, P) for _ in range(14)]


def _rng(case, what):
    return random.Random(zlib.crc32(repr((case, what)).encode()))


def case_tables(case):
    """per lookup its w columns of 2^l seeded field elements"""
    n, l, widths = CASES[case]
    rng = _rng(case, "table")
    M = 1 << l
    tables = [[[rng.randrange(P) for _ in range(M)] for _ in range(w)] for w in widths]
    if case == "dup":  # rows 2, 5, 7 hold one value: every count of it is on row 7
        tables[0][0][5] = tables[0][0][7] = tables[0][0][2]
    if case == "zeros":
        tables = [[[0] * M]]
    if case == "collide":  # two values whose Montgomery forms share their low 64 bits
        while True:
            v1 = rng.randrange(P)
            mont = v1 * _R % P
            if mont + (1 << 64) < P:
                break
        tables[0][0][1], tables[0][0][6] = v1, (mont + (1 << 64)) * _R_INV % P
    return tables


def case_rows(case):
    """per lookup the table row of every input row (what the golden file records)"""
    n, l, widths = CASES[case]
    rng = _rng(case, "rows")
    rows = [[rng.randrange(1 << l) for _ in range(1 << n)] for _ in widths]
    if case == "dup":
        rows[0][:6] = [2, 5, 7, 2, 5, 0]
    if case == "one_row":
        rows = [[3] * (1 << n)]
    if case == "collide":
        rows[0][:4] = [1, 6, 6, 1]
    return rows


def inputs_of(tables, rows):
    return [[[col[r] for r in rws] for col in table] for table, rws in zip(tables, rows)]


def case_lookups(case):
    tables = case_tables(case)
    return list(zip(inputs_of(tables, case_rows(case)), tables))
