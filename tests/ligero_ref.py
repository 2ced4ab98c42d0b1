"""Ligero PCS, restated in Python: the byte oracle of tests/test_ligero_cpu.py and tests/test_gpu_ligero.py.

The scheme is tests/brakedown_ref.py's (MultilinearBrakedown<Fr, Keccak256, _>: rows, column hashes, a Merkle tree, proximity
rows, column openings) over the other code a LinearCodes trait (util/code.rs) is expected to have: a systematic Reed-Solomon
code over the roots of unity of bn256::Fr.  This file specifies
  * the roots: w_(2^28) = 7^((r - 1) / 2^28), w_M = w_(2^28)^(2^28 / M);
  * the parameters: K = row_len = 2^row_vars, N = codeword_len = K 2^b for log_inv_rate b in 1..3, depth = row_vars + b,
    delta = 1 - 2^-b, num_column_opening = ceil(-128 / log2(1 - delta / 3)) and num_proximity_testing =
    ceil(128 / (254 - log2 N)) in IEEE double; row_vars given, or the one in 0..num_vars of the smallest
    (1 + num_proximity_testing) K + num_column_opening num_rows (the smallest on a tie);
  * the encoder: with f the polynomial of degree < K that takes m[j] at w_K^j, position i K + j of the codeword is
    f(w_N^i w_K^j): coset 0 is the message itself, K = 1 is the repetition code;
  * commit, open and verify: brakedown_ref's, restated with this encoder (test_ligero_cpu.py runs brakedown_ref's own
    functions with its encoder swapped and compares bytes).
The transforms are plain radix-2 over Python integers; field arithmetic is exact, so any correct algorithm gives these
bytes."""
import math

import numpy as np

import brakedown_ref as br
from oracle.pyref.field import R_MOD as P

PcsError, Transcript, Commitment = br.PcsError, br.Transcript, br.Commitment
TWO_ADICITY = 28
ROOT_2_28 = pow(7, (P - 1) >> TWO_ADICITY, P)
assert pow(ROOT_2_28, 1 << (TWO_ADICITY - 1), P) == P - 1  # a primitive 2^28-th root
ROW_VARS_AUTO = None


def root_of_unity(log2_m):
    assert 0 <= log2_m <= TWO_ADICITY
    return pow(ROOT_2_28, 1 << (TWO_ADICITY - log2_m), P)


def num_column_opening(b):
    delta = 1.0 - 1.0 / float(1 << b)
    return br._ceil(-br.LAMBDA / math.log2(1.0 - delta / 3.0))


def num_proximity_testing(log2_n):
    return br._ceil(br.LAMBDA / (float(br.LOG2_Q) - float(log2_n)))


def proof_elements(row_vars, num_vars, b):
    return (1 + num_proximity_testing(row_vars + b)) * (1 << row_vars) + num_column_opening(b) * (1 << (num_vars - row_vars))


def choose_row_vars(num_vars, b):
    best, row_vars = None, 0
    for rv in range(num_vars + 1):
        ps = proof_elements(rv, num_vars, b)
        if best is None or ps < best:
            best, row_vars = ps, rv
    return row_vars


class Params:
    def __init__(self, num_vars, log_inv_rate=2, row_vars=ROW_VARS_AUTO):
        if not 1 <= log_inv_rate <= 3:
            raise ValueError("log_inv_rate must be 1..3")
        if not 1 <= num_vars <= 26:
            raise ValueError("num_vars must be 1..26")
        if row_vars is ROW_VARS_AUTO:
            row_vars = choose_row_vars(num_vars, log_inv_rate)
        if row_vars > num_vars or row_vars + log_inv_rate > TWO_ADICITY:
            raise ValueError("row_vars out of range")
        self.num_vars, self.log_inv_rate, self.row_vars = num_vars, log_inv_rate, row_vars
        self.n_0 = 0
        self.row_len = 1 << row_vars
        self.codeword_len = self.row_len << log_inv_rate
        self.num_rows = 1 << (num_vars - row_vars)
        self.depth = row_vars + log_inv_rate
        self.num_column_opening = num_column_opening(log_inv_rate)
        self.num_proximity_testing = num_proximity_testing(self.depth)

    def info(self):
        return (self.row_len, self.num_rows, self.codeword_len, self.num_column_opening, self.num_proximity_testing)

    def proof_len(self):
        """bytes of one opening: the proximity and t_0 rows (or the polynomial itself when there is one row), then
        num_column_opening columns of num_rows entries with a path of depth digests each"""
        multi = self.num_rows > 1
        elems = ((1 + self.num_proximity_testing) * self.row_len if multi else self.row_len)
        return 32 * (elems + self.num_column_opening * (self.num_rows + self.depth))


# ------------------------------------------------------------------ the transforms
def ntt(values, w):
    """[sum_t values[t] w^(t s) for s], len(values) a power of two and w a primitive root of that order"""
    n = len(values)
    if n == 1:
        return list(values)
    a = list(values)
    j = 0
    for i in range(1, n):  # bit reversal
        bit = n >> 1
        while j & bit:
            j ^= bit
            bit >>= 1
        j |= bit
        if i < j:
            a[i], a[j] = a[j], a[i]
    h = 1
    while h < n:
        wh = pow(w, n // (2 * h), P)
        tw = [1] * h
        for k in range(1, h):
            tw[k] = tw[k - 1] * wh % P
        for g in range(0, n, 2 * h):
            for k in range(h):
                u, v = a[g + k], a[g + k + h] * tw[k] % P
                a[g + k], a[g + k + h] = (u + v) % P, (u - v) % P
        h *= 2
    return a


def interpolate(msg):
    """the coefficients of the f of degree < K with f(w_K^j) = msg[j]"""
    k = len(msg)
    w = root_of_unity(k.bit_length() - 1)
    k_inv = pow(k, P - 2, P)
    return [c * k_inv % P for c in ntt(msg, pow(w, P - 2, P))]


def encode(pp, msg):
    assert len(msg) == pp.row_len
    coeffs = interpolate([m % P for m in msg])
    w_n, w_k = root_of_unity(pp.depth), root_of_unity(pp.row_vars)
    out = [m % P for m in msg]
    for i in range(1, 1 << pp.log_inv_rate):
        shift, s = pow(w_n, i, P), 1
        scaled = []
        for c in coeffs:
            scaled.append(c * s % P)
            s = s * shift % P
        out += ntt(scaled, w_k)
    return out


# ------------------------------------------------------------------ commit / open / verify: brakedown_ref's, this encoder
def commit(pp, evals):
    assert len(evals) == 1 << pp.num_vars
    rows = [encode(pp, evals[r * pp.row_len:(r + 1) * pp.row_len]) for r in range(pp.num_rows)]
    width = 1 << pp.depth
    words = np.zeros((pp.codeword_len, 4 * pp.num_rows), dtype=np.uint64)
    for r, row in enumerate(rows):
        for j in range(4):
            words[:, 4 * r + j] = [(x >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for x in row]
    level = np.zeros((width, 4), dtype=np.uint64)
    level[:pp.codeword_len] = br.keccak256_words(words)
    hashes = br.digests_to_bytes(level)
    while width > 1:
        level = br.keccak256_words(level.reshape(width // 2, 8))
        hashes += br.digests_to_bytes(level)
        width //= 2
    assert len(hashes) == (2 << pp.depth) - 1
    return Commitment(rows, hashes)


def open_(pp, evals, comm, point, tr):
    row_len, num_rows = pp.row_len, pp.num_rows
    t_0, _ = br.point_to_tensor(num_rows, point)

    def combine(coeffs):
        return [sum(coeffs[r] * evals[r * row_len + c] for r in range(num_rows)) % P for c in range(row_len)]

    if num_rows > 1:
        for _ in range(pp.num_proximity_testing):
            tr.write_field_elements(combine(tr.squeeze_challenges(num_rows)))
        tr.write_field_elements(combine(t_0))
    else:
        tr.write_field_elements(evals)
    for _ in range(pp.num_column_opening):
        column = br.squeeze_challenge_idx(tr, pp.codeword_len)
        tr.write_field_elements([comm.rows[r][column] for r in range(num_rows)])
        offset = 0
        for idx in range(pp.depth):
            tr.write_hash(comm.hashes[offset + ((column >> idx) ^ 1)])
            offset += 1 << (pp.depth - idx)


def verify(vp, root, point, value, tr):
    """raises PcsError with the reference's strings"""
    row_len, num_rows = vp.row_len, vp.num_rows
    t_0, t_1 = br.point_to_tensor(num_rows, point)
    combined = []
    if num_rows > 1:
        coeffs = tr.squeeze_challenges(num_rows)
        combined.append((coeffs, encode(vp, tr.read_field_elements(row_len))))
    combined.append((t_0, encode(vp, tr.read_field_elements(row_len))))
    for _ in range(vp.num_column_opening):
        column = br.squeeze_challenge_idx(tr, vp.codeword_len)
        items = tr.read_field_elements(num_rows)
        path = [tr.read_hash() for _ in range(vp.depth)]
        for coeffs, enc in combined:
            item = sum(c * x for c, x in zip(coeffs, items)) % P if num_rows > 1 else items[0]
            if item != enc[column]:
                raise PcsError("Proximity failure")
        out = br.column_hash(items)
        for idx, sib in enumerate(path):
            h = br.FastKeccak256()
            h.update(out + sib if (column >> idx) & 1 == 0 else sib + out)
            out = h.finalize_reset()
        if out != root:
            raise PcsError("Invalid merkle tree opening")
    if sum(a * b for a, b in zip(combined[-1][1][:row_len], t_1)) % P != value % P:
        raise PcsError("Consistency failure")


def read_commitments(num, tr):
    return [tr.read_hash() for _ in range(num)]


# ------------------------------------------------------------------ the cases of tests/golden/ligero.json
# (num_vars, log_inv_rate, row_vars or None for the chosen one): every chosen shape from 3 to 10 variables at rates 1/2 and
# 1/4, forced row lengths that give 2 and 64 rows, and one case of 12 variables (4 rows of 2^10), stored in full
GOLDEN_CASES = ([(nv, b, None) for nv in range(3, 11) for b in (1, 2)] +
                [(6, 2, 5), (8, 1, 2), (10, 2, 4), (12, 2, None)])
GOLDEN_FULL = (12, 2, None)


def golden_name(case):
    return "nv%d_b%d_%s" % (case[0], case[1], "auto" if case[2] is None else "rv%d" % case[2])


def golden_proof(case):
    """-> (params, root, point, value, proof bytes) of a case: seeded random evaluations and point"""
    import random
    from oracle.pyref.poly import evaluate
    nv, b, rv = case
    pp = Params(nv, b, rv)
    rng = random.Random("ligero %d %d %r" % case)
    evals = [rng.randrange(P) for _ in range(1 << nv)]
    point = [rng.randrange(P) for _ in range(nv)]
    comm = commit(pp, evals)
    tr = Transcript()
    open_(pp, evals, comm, point, tr)
    return pp, comm.root, point, evaluate(evals, point), tr.into_proof()
