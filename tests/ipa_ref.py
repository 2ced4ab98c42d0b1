"""The multilinear IPA over BN254 G1, and Hyrax on top of it.  TEST INFRASTRUCTURE ONLY (not a test file).

A big-int restatement, written from the reference's text, of
  MultilinearIpa::{setup, trim, commit, batch_commit, open, batch_open, verify, batch_verify}   pcs/multilinear/ipa.rs:98-337
  MultilinearHyrax::{setup, trim, commit, batch_commit, open, batch_open, verify, batch_verify} pcs/multilinear/hyrax.rs:80-321
  additive::{batch_open, batch_verify}                                                        pcs/multilinear.rs:134-276
instantiated with C = bn256::G1Affine, with the module interface oracle/pyref/lasso.py `prove(..., pcs=...)` and
oracle/pyref/hyperplonk.py expect (commit, batch_commit_and_write, batch_open, batch_verify on trimmed params), as
tests/gemini_ref.py has it.

The ONE thing that is not the reference's: where the generators come from.  The reference takes g[idx] and h from the
`hash_to_curve` of a halo2curves branch whose bytes cannot be pinned here; this module (and the library)
keeps the reference's domain and messages and specifies the map itself - `hash_to_point` below.

Two ends the reference has, kept:
  * the identity cannot be written to a transcript (util/transcript.rs:172-179): a table whose upper half is zero makes
    the first L the identity, and the opening ends there with a TranscriptError;
  * a zero challenge is `invert().unwrap()` on None: ZeroDivisionError here.
A poly of fewer variables than the param is committed against a prefix of g (the commitment of its zero-padded table);
the reference's MSM asserts equal lengths there.  Openings need num_vars == the param's.
"""
from oracle.pyref.field import R_MOD as P, Q_MOD as Q, batch_invert
from oracle.pyref import curve, kzg, sum_check as sc, expression as ex
from oracle.pyref.keccak import keccak256
from oracle.pyref.poly import eq_xy, eq_xy_eval, evaluate

Evaluation = kzg.Evaluation
PcsError = kzg.PcsError
DOMAIN = b"MultilinearIpa::setup"  # ipa.rs:105,123


# ------------------------------------------------------------------ generators (own specification)
def hash_to_point(message):
    """ctr = 0, 1, ...: d0 / d1 = keccak256(DOMAIN || message || le32(ctr) || 0x00 / 0x01) (legacy 0x01 padding);
    x = le_int(d0 || d1) mod q; rhs = x^3 + 3; y = rhs^((q+1)/4); rejected when y^2 != rhs or y = 0; of y, q - y the one
    whose canonical integer is even.  (Cofactor 1: every such point is in the group.)"""
    ctr = 0
    while True:
        pre = DOMAIN + message + ctr.to_bytes(4, "little")
        x = int.from_bytes(keccak256(pre + b"\x00") + keccak256(pre + b"\x01"), "little") % Q
        rhs = (x * x * x + 3) % Q
        y = pow(rhs, (Q + 1) // 4, Q)
        if y * y % Q == rhs and y != 0:
            return (x, y if y % 2 == 0 else Q - y)
        ctr += 1


def generator_g(idx):
    """ipa.rs:107-109: message = 0x00 || le32(idx)"""
    return hash_to_point(b"\x00" + idx.to_bytes(4, "little"))


def generator_h():
    """ipa.rs:124: message = [1]"""
    return hash_to_point(b"\x01")


class Param:
    """MultilinearIpaParams (ipa.rs:25-44); prover and verifier param are the same type"""

    def __init__(self, num_vars, g, h):
        self.num_vars, self.g, self.h = num_vars, g, h


_G_CACHE = []


def setup(poly_size):
    """ipa.rs:98-127"""
    assert poly_size >= 1 and poly_size & (poly_size - 1) == 0
    while len(_G_CACHE) < poly_size:
        _G_CACHE.append(generator_g(len(_G_CACHE)))
    return Param(poly_size.bit_length() - 1, _G_CACHE[:poly_size], generator_h())


def trim(param, poly_size):
    """ipa.rs:129-145 -> (pp, vp)"""
    assert poly_size >= 1 and poly_size & (poly_size - 1) == 0
    num_vars = poly_size.bit_length() - 1
    if param.num_vars < num_vars:
        raise PcsError("Too many variates to trim (param supports variates up to %d but got %d)" % (param.num_vars, num_vars))
    p = Param(num_vars, param.g[:poly_size], param.h)
    return p, p


def _validate(function, pp, num_vars):
    """pcs/multilinear.rs:26-70"""
    if pp.num_vars < num_vars:
        raise PcsError("Too many variates of poly to %s (param supports variates up to %d but got %d)"
                       % (function, pp.num_vars, num_vars))


def commit(pp, evals):
    """ipa.rs:147-151"""
    _validate("commit", pp, len(evals).bit_length() - 1)
    return curve.msm(list(evals), pp.g[:len(evals)])


def batch_commit_and_write(pp, polys, transcript):
    comms = [commit(pp, p) for p in polys]
    transcript.write_commitments(comms)
    return comms


def _inner(a, b):
    return sum(x * y for x, y in zip(a, b)) % P


def open_(pp, evals, point, eval_, transcript):
    """ipa.rs:170-241 (`eval_` is only read by the sanity-check feature)"""
    n = pp.num_vars
    _validate("open", pp, len(point))
    assert n >= 1 and len(point) == n and len(evals) == 1 << n
    xi_0 = transcript.squeeze_challenge()
    h_prime = curve.mul(pp.h, xi_0)
    bases, coeffs, zs = list(pp.g), [v % P for v in evals], eq_xy(point)
    for i in range(n):
        mid = 1 << (n - i - 1)
        bases_l, bases_r = bases[:mid], bases[mid:]
        coeffs_l, coeffs_r = coeffs[:mid], coeffs[mid:]
        zs_l, zs_r = zs[:mid], zs[mid:]
        c_l, c_r = _inner(coeffs_r, zs_l), _inner(coeffs_l, zs_r)
        l_i = curve.msm(coeffs_r + [c_l], bases_l + [h_prime])
        r_i = curve.msm(coeffs_l + [c_r], bases_r + [h_prime])
        transcript.write_commitment(l_i)
        transcript.write_commitment(r_i)
        xi = transcript.squeeze_challenge()
        if xi == 0:
            raise ZeroDivisionError("xi_i.invert().unwrap()")
        xi_inv = pow(xi, P - 2, P)
        bases = [curve.add(l, curve.mul(r, xi)) for l, r in zip(bases_l, bases_r)]
        coeffs = [(l + xi_inv * r) % P for l, r in zip(coeffs_l, coeffs_r)]
        zs = [(l + xi * r) % P for l, r in zip(zs_l, zs_r)]
    transcript.write_field_element(coeffs[0])


def h_coeffs(scalar, xis):
    """ipa.rs:319-337"""
    assert xis
    coeffs = [scalar % P]
    for xi in reversed(xis):
        coeffs = coeffs + [c * xi % P for c in coeffs]
    return coeffs


def verify(vp, comm, point, eval_, transcript):
    """ipa.rs:269-305"""
    n = vp.num_vars
    assert len(point) == n
    xi_0 = transcript.squeeze_challenge()
    ls, rs, xis = [], [], []
    for _ in range(n):
        ls.append(transcript.read_commitment())
        rs.append(transcript.read_commitment())
        xis.append(transcript.squeeze_challenge())
    neg_c = (-transcript.read_field_element()) % P
    xi_invs = batch_invert(xis)
    neg_c_h = h_coeffs(neg_c, xis)
    u = xi_0 * (evaluate(neg_c_h, point) + eval_) % P
    acc = curve.msm(xi_invs + xis + neg_c_h + [u], ls + rs + list(vp.g) + [vp.h])
    if curve.add(acc, comm) is not None:
        raise PcsError("Invalid multilinear IPA open")


def batch_open(pp, num_vars, polys, points, evals, transcript):
    """additive::batch_open (pcs/multilinear.rs:134-235) with Pcs = MultilinearIpa; g_prime_eval is passed as zero"""
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
    """additive::batch_verify (pcs/multilinear.rs:237-276) with Pcs = MultilinearIpa"""
    ell = (len(evals) - 1).bit_length() if len(evals) > 1 else 0
    t = transcript.squeeze_challenges(ell)
    eq_xt = eq_xy(t)
    tilde_gs_sum = sum(ev.value * w for ev, w in zip(evals, eq_xt)) % P
    g_prime_eval, challenges = sc.verify(sc.Coefficients, num_vars, 2, tilde_gs_sum, transcript)
    eq_evals = [eq_xy_eval(challenges, pt) for pt in points]
    scalars = [eq_evals[ev.point] * w % P for ev, w in zip(evals, eq_xt)]
    g_prime_comm = curve.msm(scalars, [comms[ev.poly] for ev in evals])
    verify(vp, g_prime_comm, challenges, g_prime_eval, transcript)


# ------------------------------------------------------------------ MultilinearHyrax (pcs/multilinear/hyrax.rs:23-321)
class HyraxParam:
    """MultilinearHyraxParams (hyrax.rs:26-62); prover and verifier param are the same type"""

    def __init__(self, num_vars, batch_num_vars, row_num_vars, ipa):
        self.num_vars, self.batch_num_vars, self.row_num_vars, self.ipa = num_vars, batch_num_vars, row_num_vars, ipa

    @property
    def row_len(self):
        return 1 << self.row_num_vars

    @property
    def num_chunks(self):
        return 1 << (self.num_vars - self.row_num_vars)


def hyrax_dims(poly_size, batch_size):
    """hyrax.rs:122-127 -> (num_vars, batch_num_vars, row_num_vars)"""
    assert poly_size >= 1 and poly_size & (poly_size - 1) == 0
    assert 0 < batch_size <= poly_size
    batch_num_vars = (poly_size * batch_size - 1).bit_length()  # next_power_of_two().ilog2()
    return poly_size.bit_length() - 1, batch_num_vars, (batch_num_vars + 1) // 2


def hyrax_setup(poly_size, batch_size):
    """hyrax.rs:121-137"""
    num_vars, batch_num_vars, row_num_vars = hyrax_dims(poly_size, batch_size)
    return HyraxParam(num_vars, batch_num_vars, row_num_vars, setup(1 << row_num_vars))


def hyrax_trim(param, poly_size, batch_size):
    """hyrax.rs:139-167 -> (pp, vp)"""
    num_vars, batch_num_vars, row_num_vars = hyrax_dims(poly_size, batch_size)
    if param.row_num_vars < row_num_vars:
        raise PcsError("Too many variates to trim (param supports variates up to %d but got %d)"
                       % (param.row_num_vars, row_num_vars))
    p = HyraxParam(num_vars, batch_num_vars, row_num_vars, trim(param.ipa, 1 << row_num_vars)[0])
    return p, p


def hyrax_commit(pp, evals):
    """hyrax.rs:169-187 -> the list of row commitments"""
    _validate("commit", pp, len(evals).bit_length() - 1)
    assert len(evals) == 1 << pp.num_vars
    return [curve.msm(list(evals[s:s + pp.row_len]), pp.ipa.g) for s in range(0, len(evals), pp.row_len)]


def hyrax_batch_commit_and_write(pp, polys, transcript):
    """hyrax.rs:189-221, then every chunk written in order"""
    comms = [hyrax_commit(pp, p) for p in polys]
    for comm in comms:
        transcript.write_commitments(comm)
    return comms


def fix_last_vars(evals, hi):
    """poly/multilinear.rs fix_last_vars as a field identity: sum_r eq(hi)[r] * row_r"""
    w = eq_xy(hi)
    row_len = len(evals) // len(w)
    return [sum(w[r] * evals[r * row_len + c] for r in range(len(w))) % P for c in range(row_len)]


def hyrax_open(pp, evals, point, eval_, transcript):
    """hyrax.rs:224-258"""
    assert len(point) == pp.num_vars and len(evals) == 1 << pp.num_vars
    lo, hi = point[:pp.row_num_vars], point[pp.row_num_vars:]
    row = list(evals) if not hi else fix_last_vars(evals, hi)
    open_(pp.ipa, row, lo, eval_, transcript)


def hyrax_verify(vp, comm, point, eval_, transcript):
    """hyrax.rs:288-309"""
    assert len(comm) == vp.num_chunks
    lo, hi = point[:vp.row_num_vars], point[vp.row_num_vars:]
    if not hi:
        assert vp.num_chunks == 1
        row_comm = comm[0]
    else:
        row_comm = curve.msm(eq_xy(hi), list(comm))
    verify(vp.ipa, row_comm, lo, eval_, transcript)


def hyrax_batch_open(pp, num_vars, polys, points, evals, transcript):
    """additive::batch_open with Pcs = MultilinearHyrax (hyrax.rs:260-271)"""
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
    hyrax_open(pp, g_prime, challenges, 0, transcript)


def hyrax_batch_verify(vp, num_vars, comms, points, evals, transcript):
    """additive::batch_verify with sum_with_scalar chunk by chunk (hyrax.rs:80-107, 311-320)"""
    ell = (len(evals) - 1).bit_length() if len(evals) > 1 else 0
    t = transcript.squeeze_challenges(ell)
    eq_xt = eq_xy(t)
    tilde_gs_sum = sum(ev.value * w for ev, w in zip(evals, eq_xt)) % P
    g_prime_eval, challenges = sc.verify(sc.Coefficients, num_vars, 2, tilde_gs_sum, transcript)
    eq_evals = [eq_xy_eval(challenges, pt) for pt in points]
    scalars = [eq_evals[ev.point] * w % P for ev, w in zip(evals, eq_xt)]
    g_prime_comm = [curve.msm(scalars, [comms[ev.poly][k] for ev in evals]) for k in range(vp.num_chunks)]
    hyrax_verify(vp, g_prime_comm, challenges, g_prime_eval, transcript)
