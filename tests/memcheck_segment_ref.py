"""TEST INFRASTRUCTURE ONLY: read-write memory checking in segments - the argument of tests/memcheck_ref.py with the initial
image as a COMMITTED column, so that a proof can start from the memory another proof ended in.  This file is the
specification of lh_memcheck_prove_segment / lh_memcheck_verify_segment: the HIP prover reproduces these proof bytes.

Statement: as in memcheck_ref, but the image `iv` (2^l words) is private: the proof commits it, beside the final values
`fv`, and the verifier returns both commitments.  A chain of segments over one memory is consistent when every segment
verifies and segment k + 1's image commitment equals segment k's final commitment.  A column's commitment depends on the
number of variables it is committed over, nv = max(n, l): the segments of a chain share it.

Protocol: memcheck_ref's, with these differences only.

 0. C   n, l, 2                       (memcheck_ref: has_init in {0, 1} - neither verifier takes the other's proof)
 1. W   ONE write_commitments block of EIGHT: addr, rv, wv, iv, fv, rt, ft, m, each padded to nv
 2.     Init[a] = h(a, iv[a], 0)
 4. W   addr(r_N), rv(r_N), wv(r_N), rt(r_N), iv(r_M), fv(r_M), ft(r_M), rt(x), m(x)
 5.     ONE batch_open over nv variables, nine evaluations

The verifier uses the opened iv(r_M) where memcheck_ref folds the public image: no host fold, so 1 <= l < 31.
"""
import random
import zlib

from oracle.pyref import gkr, kzg
from oracle.pyref import lasso as o_lasso
from oracle.pyref.field import R_MOD as P
from oracle.pyref.poly import evaluate, identity_eval

import logup_gkr_ref as lgr
import memcheck_ref as mcr
from memcheck_ref import MemcheckError, trace_of, witness  # noqa: F401  (one error type, one witness rule)

HEADER_TAG = 2
NUM_POLYS = 8  # addr, rv, wv, iv, fv, rt, ft, m
IV, FV = 3, 4  # the two commitments a chain links
# (poly, point) of the opened evaluations, in the order they are written: points 0 = r_N, 1 = r_M, 2 = x
OPENINGS = [(0, 0), (1, 0), (2, 0), (5, 0), (3, 1), (4, 1), (6, 1), (5, 2), (7, 2)]


def _shape(n, l):
    if not 1 <= n < 31:
        raise MemcheckError("num_vars out of range")
    if not 1 <= l < 31:
        raise MemcheckError("mem_vars out of range")
    return max(n, l)


def _evals(vals):
    return [kzg.Evaluation(poly, point, v) for (poly, point), v in zip(OPENINGS, vals)]


def prove(pp, addr, rv, wv, l, image, transcript, forge=None):
    """addr, rv, wv: 2^n ints below 2^32; image: 2^l ints.  -> the final values fv (the next segment's image).
    forge (tests only): called with (addr, rv, wv, image), returns the witness dict - a cheating prover; with a key
    "iv_committed" the column committed in iv's place (everything else is done with `image`)."""
    N, M = len(addr), 1 << l
    n = N.bit_length() - 1
    assert N == 1 << n and len(rv) == N and len(wv) == N and len(image) == M
    nv = _shape(n, l)
    image = list(image)
    w = forge(addr, rv, wv, image) if forge else witness(addr, rv, wv, image)
    rt, fv, ft, m = w["rt"], w["fv"], w["ft"], w["m"]
    transcript.common_field_elements([n, l, HEADER_TAG])
    pp_nv = pp.trim(nv)
    polys = [o_lasso._pad([v % P for v in c], nv) for c in (addr, rv, wv, image, fv, rt, ft, m)]
    comms = [kzg.commit(pp_nv, p) for p in polys]
    if "iv_committed" in w:
        comms[IV] = kzg.commit(pp_nv, o_lasso._pad([v % P for v in w["iv_committed"]], nv))
    o_lasso.write_commitments(transcript, comms)

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
    at = lambda c, pt: evaluate([v % P for v in c], pt)
    vals = [at(addr, r_N), at(rv, r_N), at(wv, r_N), at(rt, r_N), at(image, r_M), at(fv, r_M), at(ft, r_M), at(rt, x), at(m, x)]
    transcript.write_field_elements(vals)
    points = [o_lasso._pad_point(pt, nv) for pt in (r_N, r_M, x)]
    kzg.batch_open(pp_nv, nv, polys, points, _evals(vals), transcript)
    return fv


def verify(vp, n, l, transcript):
    """Raises on any proof that does not verify.  -> (commitment of iv, commitment of fv), None for the identity."""
    nv = _shape(n, l)
    transcript.common_field_elements([n, l, HEADER_TAG])
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
    addr_e, rv_e, wv_e, rt_e, iv_e, fv_e, ft_e, rt_x, m_x = vals
    h = o_lasso._fingerprint
    id_N, id_M, id_x = identity_eval(r_N), identity_eval(r_M), identity_eval(x)
    want = [h(addr_e, rv_e, rt_e, gamma, tau), h(addr_e, wv_e, id_N + 1, gamma, tau), h(id_M, iv_e, 0, gamma, tau),
            h(id_M, fv_e, ft_e, gamma, tau)]
    if want != [c[0] for c in claims]:
        raise MemcheckError("leaf claim mismatch")
    if [p_x[0], q_x[0], p_x[1], q_x[1]] != [1, (delta + id_x - rt_x) % P, -m_x % P, (delta + id_x) % P]:
        raise MemcheckError("range leaf claim mismatch")
    points = [o_lasso._pad_point(pt, nv) for pt in (r_N, r_M, x)]
    kzg.batch_verify(vp.trim(nv), nv, comms, points, _evals(vals), transcript)
    if transcript.pos != len(transcript.stream):
        raise MemcheckError("trailing bytes in proof")
    return comms[IV], comms[FV]


def verify_chain(vp, l, segments, transcript_of):
    """segments: [(n, proof bytes)]; transcript_of(proof) -> a transcript.  -> (first image commitment, last final commitment)"""
    if len({max(n, l) for n, _ in segments}) > 1:
        raise MemcheckError("memcheck chain: the segments differ in max(num_vars, mem_vars)")
    first = last = None
    for k, (n, proof) in enumerate(segments):
        iv_c, fv_c = verify(vp, n, l, transcript_of(proof))
        if k == 0:
            first = iv_c
        elif iv_c != last:
            raise MemcheckError("memcheck chain: segment %d does not start where segment %d ends" % (k, k - 1))
        last = fv_c
    return first, last


# ------------------------------------------------------------------ the named cases: (n, l)
CASES = {
    "one_var": (1, 1),
    "small_mem": (5, 3),
    "big_mem": (2, 4),
    "zero_image": (4, 3),
    "loads_only": (4, 3),
    "one_cell": (4, 1),
    "edges": (3, 2),
    "mid": (13, 9),
}
SMALL = [c for c in CASES if max(CASES[c]) <= 6]  # the cases the golden SRS of six variables covers
EDGE_WORDS = mcr.EDGE_WORDS
CHAIN = (5, 5, 3)  # n, l, segments


def _rng(case, what):
    return random.Random(zlib.crc32(repr(("memcheck_segment", case, what)).encode()))


def case_image(case):
    n, l = CASES[case]
    rng = _rng(case, "image")
    if case == "zero_image":
        return [0] * (1 << l)
    if case == "edges":
        return [EDGE_WORDS[4], EDGE_WORDS[3], EDGE_WORDS[2], EDGE_WORDS[1]]
    return [rng.randrange(1 << 32) for _ in range(1 << l)]


def case_ops(case):
    """-> (addr, store, val): the operations as a front end knows them (store: 0 / 1; val: the word stored, 0 for a load)"""
    n, l = CASES[case]
    N, M = 1 << n, 1 << l
    rng = _rng(case, "ops")
    cells = [rng.randrange(M) for _ in range(N)]
    stores = [rng.randrange(1 << 32) if rng.randrange(3) else None for _ in range(N)]
    if case == "one_cell":
        cells = [0] * N
    if case == "loads_only":
        stores = [None] * N
    if case == "edges":  # every edge word stored and read back; cell 1 keeps the image's 2^31
        cells = [0, 0, 0, 0, 0, 0, 3, 3]
        stores = EDGE_WORDS + [None, EDGE_WORDS[-1], None]
    return cells, [int(s is not None) for s in stores], [s or 0 for s in stores]


def trace_from_ops(ops, image):
    addr, store, val = ops
    return trace_of([(a, v if s else None) for a, s, v in zip(addr, store, val)], image)


def case_trace(case):
    """-> (addr, rv, wv), 2^n ints each"""
    return trace_from_ops(case_ops(case), case_image(case))


def chain_image():
    rng = _rng("chain", "image")
    return [rng.randrange(1 << 32) for _ in range(1 << CHAIN[1])]


def chain_ops(k):
    n, l, _ = CHAIN
    rng = _rng("chain", ("ops", k))
    store = [int(rng.randrange(3) > 0) for _ in range(1 << n)]
    return [rng.randrange(1 << l) for _ in range(1 << n)], store, [rng.randrange(1 << 32) if s else 0 for s in store]


def chain_traces():
    """-> ([(addr, rv, wv)] per segment, [image of segment k] + [the last final values])"""
    images, traces = [chain_image()], []
    for k in range(CHAIN[2]):
        tr = trace_from_ops(chain_ops(k), images[-1])
        traces.append(tr)
        images.append(witness(*tr, images[-1])["fv"])
    return traces, images


# ------------------------------------------------------------------ three cheating provers
def forgery(name):
    """-> (n, l, image, (addr, rv, wv), forge)"""
    if name == "future_read":  # memcheck_ref's, over the committed all-zero image
        n, l, trace, forge = mcr.forgery("future_read")
        return n, l, [0, 0], trace, forge
    if name == "stale_init":
        # op 0 loads 4 from cell 0 whose image word is 3: the honest rule's columns for a trace that breaks the rule
        trace = ([0, 1, 0, 1], [4, 9, 4, 9], [4, 9, 6, 9])
        return 2, 1, [3, 9], trace, lambda addr, rv, wv, image: witness(addr, rv, wv, image, check=False)
    if name == "other_image":
        # an honest proof of a trace over [3, 9] that commits, in iv's place, the image [4, 9]: every sum-check is honest
        # about the true image, and the opening of the committed column at r_M is not iv(r_M)
        image = [3, 9]
        trace = trace_of([(0, None), (1, 5), (0, 7), (1, None)], image)

        def forge(addr, rv, wv, img):
            return dict(witness(addr, rv, wv, img), iv_committed=[4, 9])

        return 2, 1, image, trace, forge
    raise KeyError(name)


FORGERIES = {"stale_init": r"Init\*WS != RS\*Final", "other_image": "Invalid multilinear KZG open",
             "future_read": "the fractions do not sum to zero"}
