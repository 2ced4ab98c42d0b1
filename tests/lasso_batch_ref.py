"""TEST INFRASTRUCTURE ONLY: the batch Lasso argument - K tables with the same number of lookups 2^n in ONE proof - on top
of oracle/pyref/lasso.py, in the style of tests/lasso_tables_ref.py and tests/lasso_custom_ref.py (whose subtable wrappers
the cases below use).  This file is the specification of lh_lasso_prove_batch / lh_lasso_verify_batch: the HIP prover
reproduces these proof bytes.

Protocol (transcript order == proof layout); table t has c_t chunks of l_t bits and alpha_t memories, nv = max(n, max_t l_t):

 0. C   K, n, then per table l_t, c_t, alpha_t
 1. W   per table, in order: write_commitments of  a | dim | read_ts | E | final_cts  (one identity mask, then the points),
        every poly zero-padded to nv variables - the block of the table's own proof whenever that proof's nv is the same
 2. S   r[0..n) (shared);  W  v_t = a_t(r) for every t
 3. S   rho;  ONE ClassicSumCheck<EvaluationsProver> over  eq_0 * sum_t rho^t g_t(E_t,.)  with claim  sum_t rho^t v_t
        -> r_z;  W  E_t,i(r_z), table-major
 4. S   gamma, tau (shared);  ONE gkr.prove_grand_product over
          [RS, WS of every memory of every table]  (n-variable trees, table-major)
          [Init, Final of every memory of every table]  (l_t-variable trees, table-major)
        trees of equal depth end at the same point: r_N, and one r_M per distinct l
 5. W   per table  dim(r_N) | read_ts(r_N) | E(r_N) | final_cts(r_M(l_t))
 6.     ONE batch_open over nv variables: polys table-major, points  r, r_z, r_N, then r_M per distinct l in order of first
        appearance (zero-padded; r_M is not merged with r_N when l = n), evaluations table-major in lasso._evals order

The verifier mirrors lasso.check.  K = 1 is not special: its bytes differ from lasso.prove's by K and rho.
"""
import random
import zlib

import lasso_custom_ref as lcr
import lasso_tables_ref as ltr
from oracle.pyref import expression as ex
from oracle.pyref import gkr, kzg
from oracle.pyref import lasso as o_lasso
from oracle.pyref import sum_check as sc
from oracle.pyref.field import R_MOD as P
from oracle.pyref.poly import evaluate, eq_xy_eval, identity_eval

MAX_TABLES = 8


def _shape(specs, n):
    if not 1 <= len(specs) <= MAX_TABLES:
        raise o_lasso.LassoError("1 to %d tables" % MAX_TABLES)
    for spec in specs:
        o_lasso._check_shape(spec, n)
    ls = []
    for spec in specs:
        if spec.l not in ls:
            ls.append(spec.l)
    return max([n] + ls), ls


def surge_expression(specs, rho):
    """eq_0 * sum_t rho^t g_t over the poly list E_0,. | E_1,. | .. (table-major)"""
    terms, base, power = [], 0, 1
    for spec in specs:
        for coeff, mono in spec.g_terms:
            e = ex.Poly(base + mono[0])
            for i in mono[1:]:
                e = e * ex.Poly(base + i)
            terms.append(e * (coeff * power % P))
        base += spec.alpha
        power = power * rho % P
    return ex.EqXY(0) * ex.sum_exprs(terms)


def _batch_evals(specs, ls, vals):
    """lasso._evals per table with the poly indices shifted behind the earlier tables' polys and r_M -> 3 + index of l"""
    out, base = [], 0
    for spec, v in zip(specs, vals):
        for e in o_lasso._evals(spec, *v):
            out.append(kzg.Evaluation(base + e.poly, 3 + ls.index(spec.l) if e.point == 3 else e.point, e.value))
        base += 1 + 3 * spec.c + spec.alpha
    return out


def prove(pp, specs, dims_list, transcript):
    """specs: K TableSpec; dims_list[t]: c_t lists of 2^n chunk indices"""
    N = len(dims_list[0][0])
    n = N.bit_length() - 1
    assert N == 1 << n and len(specs) == len(dims_list)
    assert all(len(d) == N for dims in dims_list for d in dims) and all(len(dims) == s.c for s, dims in zip(specs, dims_list))
    nv, ls = _shape(specs, n)
    ws = [o_lasso.witness(spec, dims) for spec, dims in zip(specs, dims_list)]
    transcript.common_field_elements([len(specs), n])
    for spec in specs:
        transcript.common_field_elements([spec.l, spec.c, spec.alpha])
    pp_nv = pp.trim(nv)
    polys = []
    for w in ws:
        block = [o_lasso._pad(p, nv) for p in [w["a"]] + w["dim"] + w["read_ts"] + w["E"] + w["final_cts"]]
        o_lasso.write_commitments(transcript, [kzg.commit(pp_nv, p) for p in block])
        polys += block

    r = transcript.squeeze_challenges(n)
    vs = [evaluate(w["a"], r) for w in ws]
    transcript.write_field_elements(vs)
    rho = transcript.squeeze_challenge()
    claim, power = 0, 1
    for v in vs:
        claim = (claim + power * v) % P
        power = power * rho % P
    vp = sc.VirtualPolynomial(surge_expression(specs, rho), [e for w in ws for e in w["E"]], [], [r])
    r_z, e_rz = sc.prove(sc.EvaluationsProver, n, vp, claim, transcript)
    transcript.write_field_elements(e_rz)

    gamma = transcript.squeeze_challenge()
    tau = transcript.squeeze_challenge()
    fp = o_lasso._fingerprint
    leaves_n, leaves_l = [], []
    for spec, w in zip(specs, ws):
        M = 1 << spec.l
        for i, (j, kind) in enumerate(spec.memories):
            rs = [fp(w["dim"][j][k], w["E"][i][k], w["read_ts"][j][k], gamma, tau) for k in range(N)]
            init = [fp(m, o_lasso.subtable_entry(kind, m, spec.l), 0, gamma, tau) for m in range(M)]
            leaves_n += [rs, [(x + 1) % P for x in rs]]
            leaves_l += [init, [(init[m] + w["final_cts"][j][m]) % P for m in range(M)]]
    _, claims = gkr.prove_grand_product(leaves_n + leaves_l, transcript)
    r_N = claims[0][1]
    r_M, pos = {}, len(leaves_n)
    for spec in specs:
        r_M.setdefault(spec.l, claims[pos][1])
        assert claims[pos][1] == r_M[spec.l]
        pos += 2 * spec.alpha

    vals, at = [], 0
    for spec, w, v in zip(specs, ws, vs):
        dim_e = [evaluate(t, r_N) for t in w["dim"]]
        rts_e = [evaluate(t, r_N) for t in w["read_ts"]]
        e_e = [evaluate(t, r_N) for t in w["E"]]
        fc_e = [evaluate(t, r_M[spec.l]) for t in w["final_cts"]]
        transcript.write_field_elements(dim_e + rts_e + e_e + fc_e)
        vals.append((v, e_rz[at:at + spec.alpha], dim_e, rts_e, e_e, fc_e))
        at += spec.alpha
    points = [o_lasso._pad_point(pt, nv) for pt in [r, r_z, r_N] + [r_M[l] for l in ls]]
    kzg.batch_open(pp_nv, nv, polys, points, _batch_evals(specs, ls, vals), transcript)
    return transcript


def verify(vp, specs, n, transcript):
    nv, ls = _shape(specs, n)
    transcript.common_field_elements([len(specs), n])
    for spec in specs:
        transcript.common_field_elements([spec.l, spec.c, spec.alpha])
    comms = []
    for spec in specs:
        comms += o_lasso.read_commitments(transcript, 1 + 3 * spec.c + spec.alpha)
    r = transcript.squeeze_challenges(n)
    vs = transcript.read_field_elements(len(specs))
    rho = transcript.squeeze_challenge()
    claim, power = 0, 1
    for v in vs:
        claim = (claim + power * v) % P
        power = power * rho % P
    degree = 1 + max(len(mono) for spec in specs for _, mono in spec.g_terms)
    x_eval, r_z = sc.verify(sc.Evaluations, n, degree, claim, transcript)
    e_rz = transcript.read_field_elements(sum(spec.alpha for spec in specs))
    want, power, at = 0, 1, 0
    for spec in specs:
        want = (want + power * spec.g_eval(e_rz[at:at + spec.alpha])) % P
        power = power * rho % P
        at += spec.alpha
    if x_eval != eq_xy_eval(r_z, r) * want % P:
        raise o_lasso.LassoError("Surge sum-check final evaluation mismatch")

    gamma = transcript.squeeze_challenge()
    tau = transcript.squeeze_challenge()
    total = sum(spec.alpha for spec in specs)
    roots, claims = gkr.verify_grand_product([n] * (2 * total) + [spec.l for spec in specs for _ in range(2 * spec.alpha)],
                                             transcript)
    for i in range(total):
        rs, ws, init, final = roots[2 * i], roots[2 * i + 1], roots[2 * total + 2 * i], roots[2 * total + 2 * i + 1]
        if init * ws % P != rs * final % P:
            raise o_lasso.LassoError("memory %d: Init*WS != RS*Final" % i)
    r_N = claims[0][1]
    r_M, pos = {}, 2 * total
    for spec in specs:
        r_M.setdefault(spec.l, claims[pos][1])
        pos += 2 * spec.alpha

    fp = o_lasso._fingerprint
    vals, base, at = [], 0, 0
    for spec, v in zip(specs, vs):
        c, alpha = spec.c, spec.alpha
        got = transcript.read_field_elements(3 * c + alpha)
        dim_e, rts_e, e_e, fc_e = got[:c], got[c:2 * c], got[2 * c:2 * c + alpha], got[2 * c + alpha:]
        pt = r_M[spec.l]
        id_M = identity_eval(pt)
        for i, (j, kind) in enumerate(spec.memories):
            rs = fp(dim_e[j], e_e[i], rts_e[j], gamma, tau)
            init = fp(id_M, o_lasso.subtable_mle_eval(kind, pt), 0, gamma, tau)
            b = base + i
            if [rs, (rs + 1) % P, init, (init + fc_e[j]) % P] != \
                    [claims[2 * b][0], claims[2 * b + 1][0], claims[2 * total + 2 * b][0], claims[2 * total + 2 * b + 1][0]]:
                raise o_lasso.LassoError("memory %d: leaf claim mismatch" % b)
        vals.append((v, e_rz[at:at + alpha], dim_e, rts_e, e_e, fc_e))
        base += alpha
        at += alpha
    points = [o_lasso._pad_point(pt, nv) for pt in [r, r_z, r_N] + [r_M[l] for l in ls]]
    kzg.batch_verify(vp.trim(nv), nv, comms, points, _batch_evals(specs, ls, vals), transcript)
    if transcript.pos != len(transcript.stream):
        raise o_lasso.LassoError("trailing bytes in proof")


# ------------------------------------------------------------------ the named cases
# a table: ("range", c, l) | ("and" / "xor", c, l) | ("less_than" / "equal", c, l) | ("custom", name of lasso_custom_ref.TABLES, c)
CUSTOM_KIND = lcr.CUSTOM_BASE + 11  # (any custom kind: it is not absorbed into the transcript)
CASES = {
    "two_ranges": (4, [("range", 2, 2), ("range", 2, 3)]),
    "and_xor_shared": (5, [("and", 2, 4), ("xor", 2, 4)]),
    "pad": (2, [("range", 1, 3), ("and", 2, 4)]),
    "mixed_g": (4, [("less_than", 2, 4), ("range", 2, 2)]),
    "single": (3, [("equal", 2, 4)]),
    "custom": (4, [("custom", "rand1", 2), ("range", 2, 3)]),
    "zeros": (4, [("and", 2, 4), ("range", 2, 3)]),
    "full": (5, [("and", 4, 4), ("and", 4, 4)]),
}
SHARED = {"and_xor_shared"}  # cases whose tables all read the FIRST table's chunk columns


def spec_of(desc, kind=CUSTOM_KIND):
    name, c, l = desc
    if name == "range":
        return o_lasso.range_table(c, l)
    if name in ("and", "xor"):
        return o_lasso.bitwise_table(o_lasso.SUBTABLE_AND if name == "and" else o_lasso.SUBTABLE_XOR, c, l)
    if name in ("less_than", "equal"):
        return ltr.spec_of(name, c, l)
    return lcr.spec_of(c, l, "linear", kind)  # (("custom", name of the table, chunks): c holds the name, l the chunks)


def table_of(hl, desc, kind=None):
    name, c, l = desc
    if name == "range":
        return hl.LassoTable.range(c, l)
    if name in ("and", "xor"):
        return hl.LassoTable.bitwise(hl.SUBTABLE_AND if name == "and" else hl.SUBTABLE_XOR, c, l)
    if name in ("less_than", "equal"):
        return ltr.table_of(hl, name, c, l)
    return lcr.table_of(hl, c, l, "linear", kind)  # (as in spec_of)


def custom_values(case):
    """{kind: values} for lasso_custom_ref.installed: the registered tables a case needs"""
    return {CUSTOM_KIND: lcr.TABLES[d[1]] for d in CASES[case][1] if d[0] == "custom"}


def case_dims(case):
    """seeded chunk columns of every table of a case (lists of lists); a SHARED case returns the same list objects twice"""
    n, descs = CASES[case]
    out = []
    for t, desc in enumerate(descs):
        spec = spec_of(desc)
        if case in SHARED and t:
            out.append(out[0])
            continue
        rng = random.Random(zlib.crc32(repr((case, t, n)).encode()))
        dims = [[rng.randrange(1 << spec.l) for _ in range(1 << n)] for _ in range(spec.c)]
        if case == "zeros":
            h = spec.l // 2
            if desc[0] == "and":  # operands that share no bit: E = 0 everywhere
                for d in dims:
                    for k, m in enumerate(d):
                        x = m >> h
                        d[k] = x << h | ((m & ((1 << h) - 1)) & ~x)
            else:  # a range whose high chunk is all zero
                dims[-1] = [0] * (1 << n)
        out.append(dims)
    return out
