"""TEST INFRASTRUCTURE ONLY: read-write memory checking - a stand-alone argument for RAM traces - on top of oracle/pyref
(gkr.prove_grand_product, gkr.prove_fractional_sum_check, kzg, lasso.write_commitments) and the restated fractional verifier
of tests/logup_gkr_ref.py.  This file is the specification of lh_memcheck_prove / lh_memcheck_verify: the HIP prover
reproduces these proof bytes.

Statement: a memory of 2^l cells of 32-bit words with a PUBLIC initial image `init` (None: all zero; part of the statement,
not absorbed into the transcript) and a trace of 2^n operations (addr, rv, wv): cell addr[i] held rv[i] before operation i
and holds wv[i] after it (a load: wv = rv).  Claim: addr[i] < 2^l, and rv[i] is the wv of the latest earlier operation on
the same cell, or init[addr[i]] when there is none.  Operation i writes at time i + 1; the image has time 0.  nv = max(n, l).

Protocol (transcript order == proof layout):

 0. C   n, l, has_init
 1.     rt[i] = time of the previous write to addr[i] (0: none); fv[a], ft[a] = final value and time of cell a;
        m[d] = #{i : i - rt[i] = d}, d < 2^n.  An inconsistent trace: MemcheckError "Invalid memory trace".
    W   ONE write_commitments block: addr, rv, wv, rt, fv, ft, m, each padded to nv
 2. S   gamma, tau;  h(a, v, t) = a gamma^2 + v gamma + t - tau
        RS[i] = h(addr, rv, rt), WS[i] = h(addr, wv, i + 1), Init[a] = h(a, init[a], 0), Final[a] = h(a, fv[a], ft[a])
        gkr.prove_grand_product([RS, WS, Init, Final]) -> r_N, r_M
 3. S   delta;  ONE gkr.prove_fractional_sum_check, two fractions over n variables, roots written:
        1 / (delta + i - rt[i])   and   -m[i] / (delta + i)   -> x
 4. W   addr(r_N), rv(r_N), wv(r_N), rt(r_N), fv(r_M), ft(r_M), rt(x), m(x)
 5.     ONE batch_open over nv variables: polys in commitment order, points r_N, r_M, x zero-padded, evaluations in the
        order of step 4

The verifier mirrors this: Init WS = RS Final on the roots; Q_0 != 0, Q_1 != 0, P_0 Q_1 + P_1 Q_0 = 0 on the fractions'
roots (the LogUp range check i - rt[i] in [0, 2^n): no read from the future - without it the multiset check is unsound);
the final claims with id(.) = identity_eval and the image's multilinear extension; batch_verify; no byte left.
"""
import random
import zlib

from oracle.pyref import gkr, kzg
from oracle.pyref import lasso as o_lasso
from oracle.pyref.field import R_MOD as P
from oracle.pyref.poly import evaluate, identity_eval

import logup_gkr_ref as lgr

MAX_INIT_VARS = 24
NUM_POLYS = 7  # addr, rv, wv, rt, fv, ft, m
# (poly, point) of the opened evaluations, in the order they are written: points 0 = r_N, 1 = r_M, 2 = x
OPENINGS = [(0, 0), (1, 0), (2, 0), (3, 0), (4, 1), (5, 1), (3, 2), (6, 2)]


class MemcheckError(Exception):
    pass


def _shape(n, l, has_init):
    if not 1 <= n < 31:
        raise MemcheckError("num_vars out of range")
    if not (1 <= l <= MAX_INIT_VARS if has_init else 1 <= l < 31):
        raise MemcheckError("mem_vars out of range")
    return max(n, l)


def witness(addr, rv, wv, image, check=True):
    """-> dict(rt, fv, ft, m); check=False (tests only): the same rule without the refusal"""
    N, M = len(addr), len(image)
    fv, ft = list(image), [0] * M
    rt, m = [0] * N, [0] * N
    for i in range(N):
        a = addr[i]
        if check and (a >= M or rv[i] != fv[a]):
            raise MemcheckError("Invalid memory trace")
        rt[i] = ft[a]
        fv[a], ft[a] = wv[i], i + 1
        m[i - rt[i]] += 1
    return dict(rt=rt, fv=fv, ft=ft, m=m)


def _evals(vals):
    return [kzg.Evaluation(poly, point, v) for (poly, point), v in zip(OPENINGS, vals)]


def prove(pp, addr, rv, wv, l, init, transcript, forge=None):
    """addr, rv, wv: 2^n ints below 2^32; init: 2^l ints or None.
    forge (tests only): called with (addr, rv, wv, image), returns the witness dict - a cheating prover."""
    N, M = len(addr), 1 << l
    n = N.bit_length() - 1
    assert N == 1 << n and len(rv) == N and len(wv) == N and (init is None or len(init) == M)
    nv = _shape(n, l, init is not None)
    image = list(init) if init is not None else [0] * M
    w = forge(addr, rv, wv, image) if forge else witness(addr, rv, wv, image)
    rt, fv, ft, m = w["rt"], w["fv"], w["ft"], w["m"]
    transcript.common_field_elements([n, l, int(init is not None)])
    pp_nv = pp.trim(nv)
    polys = [o_lasso._pad([v % P for v in c], nv) for c in (addr, rv, wv, rt, fv, ft, m)]
    o_lasso.write_commitments(transcript, [kzg.commit(pp_nv, p) for p in polys])

    gamma = transcript.squeeze_challenge()
    tau = transcript.squeeze_challenge()
    h = o_lasso._fingerprint
    rs = [h(addr[i], rv[i], rt[i], gamma, tau) for i in range(N)]
    ws = [h(addr[i], wv[i], i + 1, gamma, tau) for i in range(N)]
    ini = [h(a, image[a], 0, gamma, tau) for a in range(M)]
    fin = [h(a, fv[a], ft[a], gamma, tau) for a in range(M)]
    _, claims = gkr.prove_grand_product([rs, ws, ini, fin], transcript)
    r_N, r_M = claims[0][1], claims[2][1]

    delta = transcript.squeeze_challenge()
    none = [None, None]
    _, _, x = gkr.prove_fractional_sum_check(none, none, [[1] * N, [-c % P for c in m]],
                                             [[(delta + i - rt[i]) % P for i in range(N)], [(delta + i) % P for i in range(N)]],
                                             transcript)
    at_n = lambda c, pt: evaluate([v % P for v in c], pt)
    vals = [at_n(addr, r_N), at_n(rv, r_N), at_n(wv, r_N), at_n(rt, r_N), at_n(fv, r_M), at_n(ft, r_M), at_n(rt, x), at_n(m, x)]
    transcript.write_field_elements(vals)
    points = [o_lasso._pad_point(pt, nv) for pt in (r_N, r_M, x)]
    kzg.batch_open(pp_nv, nv, polys, points, _evals(vals), transcript)
    return transcript


def verify(vp, n, l, init, transcript):
    """Raises on any proof that does not verify."""
    nv = _shape(n, l, init is not None)
    assert init is None or len(init) == 1 << l
    transcript.common_field_elements([n, l, int(init is not None)])
    comms = o_lasso.read_commitments(transcript, NUM_POLYS)
    gamma = transcript.squeeze_challenge()
    tau = transcript.squeeze_challenge()
    roots, claims = gkr.verify_grand_product([n, n, l, l], transcript)
    if roots[2] * roots[1] % P != roots[0] * roots[3] % P:
        raise MemcheckError("Init*WS != RS*Final")
    r_N, r_M = claims[0][1], claims[2][1]
    delta = transcript.squeeze_challenge()
    p_0, q_0, p_x, q_x, x = lgr.verify_fractional_sum_check(n, 2, transcript)
    if q_0[0] == 0 or q_0[1] == 0 or (p_0[0] * q_0[1] + p_0[1] * q_0[0]) % P:
        raise MemcheckError("the fractions do not sum to zero")
    vals = transcript.read_field_elements(len(OPENINGS))
    addr_e, rv_e, wv_e, rt_e, fv_e, ft_e, rt_x, m_x = vals
    h = o_lasso._fingerprint
    id_N, id_M, id_x = identity_eval(r_N), identity_eval(r_M), identity_eval(x)
    init_e = evaluate([v % P for v in init], r_M) if init is not None else 0
    want = [h(addr_e, rv_e, rt_e, gamma, tau), h(addr_e, wv_e, id_N + 1, gamma, tau), h(id_M, init_e, 0, gamma, tau),
            h(id_M, fv_e, ft_e, gamma, tau)]
    if want != [c[0] for c in claims]:
        raise MemcheckError("leaf claim mismatch")
    if [p_x[0], q_x[0], p_x[1], q_x[1]] != [1, (delta + id_x - rt_x) % P, -m_x % P, (delta + id_x) % P]:
        raise MemcheckError("range leaf claim mismatch")
    points = [o_lasso._pad_point(pt, nv) for pt in (r_N, r_M, x)]
    kzg.batch_verify(vp.trim(nv), nv, comms, points, _evals(vals), transcript)
    if transcript.pos != len(transcript.stream):
        raise MemcheckError("trailing bytes in proof")


# ------------------------------------------------------------------ the named cases: (n, l, has_init)
CASES = {
    "one_var": (1, 1, False),
    "small_mem": (5, 3, True),
    "big_mem": (2, 4, True),
    "square": (6, 6, False),
    "one_cell": (4, 1, True),
    "distinct": (3, 4, True),
    "loads_only": (4, 3, True),
    "edges": (3, 2, True),
    "mid": (13, 9, True),
    "wide": (9, 12, True),  # more cells than operations: the cell side's leaves come with the level above them
}
SMALL = [c for c in CASES if max(CASES[c][:2]) <= 6]  # the cases the golden SRS of six variables covers
EDGE_WORDS = [0, 1, 1 << 16, 1 << 31, (1 << 32) - 1]


def _rng(case, what):
    return random.Random(zlib.crc32(repr(("memcheck", case, what)).encode()))


def case_init(case):
    n, l, has_init = CASES[case]
    if not has_init:
        return None
    rng = _rng(case, "init")
    return [rng.randrange(1 << 32) for _ in range(1 << l)]


def trace_of(ops, image):
    """(addr, rv, wv) of a list of (cell, word to store or None for a load) over a copy of `image`"""
    mem = list(image)
    addr, rv, wv = [], [], []
    for a, store in ops:
        addr.append(a), rv.append(mem[a])
        if store is not None:
            mem[a] = store
        wv.append(mem[a])
    return addr, rv, wv


def case_trace(case):
    """-> (addr, rv, wv), 2^n ints each: what the golden file records"""
    n, l, has_init = CASES[case]
    N, M = 1 << n, 1 << l
    rng = _rng(case, "trace")
    cells = [rng.randrange(M) for _ in range(N)]
    stores = [rng.randrange(1 << 32) if rng.randrange(3) else None for _ in range(N)]
    if case == "one_cell":
        cells = [0] * N
    if case == "distinct":
        cells = rng.sample(range(M), N)
    if case == "loads_only":
        stores = [None] * N
    if case == "edges":  # every edge word stored and read back: as the rv of the store over it, the last one by a load
        cells = [0, 0, 0, 0, 0, 0, 3, 3]
        stores = EDGE_WORDS + [None, EDGE_WORDS[-1], None]
    image = case_init(case) or [0] * M
    return trace_of(list(zip(cells, stores)), image)


# ------------------------------------------------------------------ two cheating provers: (n, l, addr, rv, wv, forge)
def forgery(name):
    """-> (n, l, (addr, rv, wv), forge); no initial image"""
    if name == "future_read":
        # op 0 loads 7 from cell 0 'written' at time 2; op 1 stores that 7 over the image's 0.  With Final[0] = (7, time 1)
        # Init u WS = RS u Final as multisets: only the range check of i - rt[i] stands in the way
        trace = ([0, 0, 1, 1], [7, 0, 0, 9], [7, 7, 9, 9])

        def forge(addr, rv, wv, image):
            rt = [2, 0, 0, 3]  # (cell 1 honestly: stored at time 3, loaded at time 4)
            m = [0] * 4
            for i, t in enumerate(rt):
                m[(i - t) % 4] += 1  # the difference -2 counted somewhere: no m makes the fractions cancel
            return dict(rt=rt, fv=[7, 9], ft=[1, 4], m=m)

        return 2, 1, trace, forge
    if name == "stale_read":
        # op 2 loads the 5 that op 1 has overwritten with 6: the honest rule's columns for a trace that breaks the rule
        trace = ([0, 0, 0, 1, 1, 0, 1, 0], [0, 5, 5, 0, 8, 5, 8, 5], [5, 6, 5, 8, 8, 5, 8, 5])
        return 3, 1, trace, lambda addr, rv, wv, image: witness(addr, rv, wv, image, check=False)
    raise KeyError(name)


FORGERIES = {"future_read": "the fractions do not sum to zero", "stale_read": r"Init\*WS != RS\*Final"}
