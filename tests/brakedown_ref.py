"""Brakedown PCS, restated in Python: the byte oracle of tests/test_brakedown_cpu.py and tests/test_gpu_brakedown.py.

An independent restatement, from the reference's description, of
  * the code parameters of util/code/brakedown.rs (BrakedownSpec1..6, LAMBDA 128, log2_q 254), in IEEE double;
  * this library's matrix sampler (a Keccak-256 counter-mode word stream from a 32-byte seed);
  * the expander-code encoder (brakedown.rs:88-125);
  * MultilinearBrakedown<Fr, Keccak256, _> commit, open and verify (pcs/multilinear/brakedown.rs:89-435).
It reads oracle.pyref (field, keccak, transcript, poly) and changes none of it.  Hash commitments go through
`write_hash` / `read_hash`: raw 32 bytes in the stream, not absorbed (util/transcript.rs:240-265).
Batches of independent hashes (sampler blocks, column leaves, tree levels) run through a numpy Keccak-f.
"""
import math

import numpy as np

from oracle.pyref.field import R_MOD as P, to_repr_le
from oracle.pyref.keccak import Keccak256, RATE, _RC
from oracle.pyref.poly import eq_xy
from oracle.pyref.transcript import Keccak256Transcript, TranscriptError

LAMBDA = 128.0
LOG2_Q = 254
# Figure 2 of GLSTW21 (code/brakedown.rs:253-260): (alpha, beta, r)
SPECS = {
    1: (0.1195, 0.0284, 1.420),
    2: (0.1380, 0.0444, 1.470),
    3: (0.1780, 0.0610, 1.521),
    4: (0.2000, 0.0820, 1.640),
    5: (0.2110, 0.0970, 1.616),
    6: (0.2380, 0.1205, 1.720),
}


class PcsError(Exception):
    pass


# ------------------------------------------------------------------ parameters
def _ceil(v):
    return max(0, int(math.ceil(v)))  # `v.ceil() as usize` saturates at 0


def _h(p):
    assert 0.0 < p < 1.0
    q = 1.0 - p
    return -p * math.log2(p) - q * math.log2(q)


class Spec:
    def __init__(self, k):
        self.k = k
        self.alpha, self.beta, self.r = SPECS[k]

    def delta(self):
        return self.beta / self.r

    def mu(self):
        return self.r - 1.0 - self.r * self.alpha

    def nu(self):
        return self.beta + self.alpha * self.beta + 0.03

    def c_n(self, n):
        a, b, n = self.alpha, self.beta, float(n)
        return min(max(_ceil(1.28 * b * n), _ceil(b * n) + 4),
                   _ceil(((110.0 / n) + _h(b) + a * _h(1.28 * b / a)) / (b * math.log2(a / (1.28 * b)))))

    def d_n(self, log2_q, n):
        a, b, r, mu, nu, n = self.alpha, self.beta, self.r, self.mu(), self.nu(), float(n)
        return min(_ceil((2.0 * b + ((r - 1.0) + 110.0 / n) / float(log2_q)) * n),
                   _ceil((r * a * _h(b / r) + mu * _h(nu / mu) + 110.0 / n) / (a * b * math.log2(mu / nu))))

    def num_column_opening(self):
        return _ceil(-LAMBDA / math.log2(1.0 - self.delta() / 3.0))

    def num_proximity_testing(self, log2_q, n, n_0):
        return _ceil(LAMBDA / (float(log2_q) - math.log2(float(self.codeword_len(log2_q, n, n_0)))))

    def dimensions(self, log2_q, n, n_0):
        """([(n, m, d)] of a, [(n, m, d)] of b)"""
        assert n > n_0
        a, cur = [], n
        while True:
            nxt = _ceil(cur * self.alpha)
            if cur <= n_0:
                break
            a.append((cur, nxt, min(self.c_n(cur), nxt)))
            cur = nxt
        b = []
        for an, am, _ in a:
            n_prime = _ceil(am * self.r)
            m_prime = _ceil(an * self.r) - an - n_prime
            if m_prime < 0:
                raise PcsError("code dimensions underflow")
            b.append((n_prime, m_prime, min(self.d_n(log2_q, an), m_prime)))
        return a, b

    def codeword_len(self, log2_q, n, n_0):
        a, b = self.dimensions(log2_q, n, n_0)
        return a[0][0] + sum(m for _, m, _ in a[:-1]) + b[-1][0] + sum(m for _, m, _ in b)


def proof_size(spec, n_0, c, r):
    return (1 + spec.num_proximity_testing(LOG2_Q, c, n_0)) * c + spec.num_column_opening() * r


def choose_row_len(spec, num_vars, n_0):
    min_log2_n = (n_0 + 1 - 1).bit_length()  # (n_0 + 1).next_power_of_two().ilog2()
    best, row_len = None, 0
    for log2_n in range(min_log2_n, num_vars + 1):
        ps = proof_size(spec, n_0, 1 << log2_n, 1 << (num_vars - log2_n))
        if best is None or ps < best:
            best, row_len = ps, 1 << log2_n
    return row_len


class Params:
    """MultilinearBrakedownParams (pcs/multilinear/brakedown.rs:35-41) and the code of Brakedown::new_multilinear"""

    def __init__(self, num_vars, spec_k, seed=None):
        spec = Spec(spec_k)
        self.num_vars, self.spec = num_vars, spec
        self.n_0 = min(20, (1 << num_vars) - 1)
        self.row_len = choose_row_len(spec, num_vars, self.n_0)
        self.num_rows = (1 << num_vars) // self.row_len
        self.a_dims, self.b_dims = spec.dimensions(LOG2_Q, self.row_len, self.n_0)
        self.codeword_len = spec.codeword_len(LOG2_Q, self.row_len, self.n_0)
        self.num_column_opening = spec.num_column_opening()
        self.num_proximity_testing = spec.num_proximity_testing(LOG2_Q, self.row_len, self.n_0)
        self.depth = (self.codeword_len - 1).bit_length()
        self.a = self.b = None
        if seed is not None:
            self.a, self.b = sample_matrices(seed, self.a_dims, self.b_dims)

    def info(self):
        return (self.row_len, self.num_rows, self.codeword_len, self.num_column_opening, self.num_proximity_testing)


# ------------------------------------------------------------------ Keccak-f over many states (numpy)
_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)
_RHO = [0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14]  # lane x + 5y


def _rol_np(v, n):
    if n == 0:
        return v
    return (v << np.uint64(n)) | (v >> np.uint64(64 - n))


def keccak_f_many(a):
    """a: list of 25 uint64 arrays (lane x + 5y), permuted in place"""
    for rc in _RC:
        c = [a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20] for x in range(5)]
        d = [c[(x + 4) % 5] ^ _rol_np(c[(x + 1) % 5], 1) for x in range(5)]
        b = [None] * 25
        for x in range(5):
            for y in range(5):
                b[y + 5 * ((2 * x + 3 * y) % 5)] = _rol_np(a[x + 5 * y] ^ d[x], _RHO[x + 5 * y])
        for y in range(5):
            for x in range(5):
                a[x + 5 * y] = b[x + 5 * y] ^ ((b[(x + 1) % 5 + 5 * y] ^ _M64) & b[(x + 2) % 5 + 5 * y])
        a[0] = a[0] ^ np.uint64(rc)
    return a


def keccak256_words(words):
    """Keccak-256 of N messages of equal length, given as an (N, w) uint64 array of little-endian words;
    returns an (N, 4) uint64 array of digest words"""
    words = np.ascontiguousarray(words, dtype=np.uint64)
    n, w = words.shape
    lanes = RATE // 8
    state = [np.zeros(n, dtype=np.uint64) for _ in range(25)]
    total = w // lanes + 1
    for blk in range(total):
        chunk = words[:, blk * lanes:(blk + 1) * lanes]
        for i in range(chunk.shape[1]):
            state[i] = state[i] ^ chunk[:, i]
        if blk == total - 1:
            k = chunk.shape[1]
            state[k] = state[k] ^ np.uint64(0x01)
            state[lanes - 1] = state[lanes - 1] ^ np.uint64(0x80 << 56)
        keccak_f_many(state)
    return np.stack(state[:4], axis=1)


def digests_to_bytes(d):
    return [bytes(row.astype("<u8").tobytes()) for row in d]


# ------------------------------------------------------------------ the sampler
class WordStream:
    """block i = keccak256(seed || le64(i)), read as four little-endian u64 words"""

    def __init__(self, seed, batch=4096):
        assert len(seed) == 32
        self.seed = np.frombuffer(bytes(seed), dtype="<u8").astype(np.uint64)
        self.batch, self.next_block, self.buf, self.pos = batch, 0, [], 0

    def _refill(self):
        idx = np.arange(self.next_block, self.next_block + self.batch, dtype=np.uint64)
        msg = np.empty((self.batch, 5), dtype=np.uint64)
        msg[:, :4] = self.seed
        msg[:, 4] = idx
        self.buf = [int(v) for v in keccak256_words(msg).reshape(-1)]
        self.pos = 0
        self.next_block += self.batch

    def word(self):
        if self.pos == len(self.buf):
            self._refill()
        w = self.buf[self.pos]
        self.pos += 1
        return w

    def uniform(self, m):
        limit = ((1 << 64) // m) * m
        while True:
            w = self.word()
            if w < limit:
                return w % m

    def field(self):
        v = 0
        for j in range(8):
            v |= self.word() << (64 * j)
        return v % P


def sample_matrix(ws, dim):
    """SparseMatrix::new (code/brakedown.rs:279-297): rows[i] = [(column, coeff)] with d distinct sorted columns"""
    n, m, d = dim
    rows = []
    for _ in range(n):
        cols = set()
        while len(cols) < d:
            cols.add(ws.uniform(m))
        rows.append([(c, ws.field()) for c in sorted(cols)])
    return rows


def sample_matrices(seed, a_dims, b_dims):
    ws = WordStream(seed)
    a, b = [], []
    for ad, bd in zip(a_dims, b_dims):  # a[0], b[0], a[1], b[1], ...
        a.append(sample_matrix(ws, ad))
        b.append(sample_matrix(ws, bd))
    return a, b


# ------------------------------------------------------------------ encoder (code/brakedown.rs:88-125)
def _dot_into(rows, src, target, out_off):
    for item, cells in zip(src, rows):
        if item:
            for col, coeff in cells:
                target[out_off + col] = (target[out_off + col] + item * coeff) % P


def _horner(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % P
    return acc


def encode(pp, msg):
    assert len(msg) == pp.row_len
    t = list(msg) + [0] * (pp.codeword_len - pp.row_len)
    a_dims, b_dims = pp.a_dims, pp.b_dims
    off = 0
    for k in range(len(a_dims) - 1):
        n = a_dims[k][0]
        _dot_into(pp.a[k], t[off:off + n], t, off + n)
        off += n
    an, am, _ = a_dims[-1]
    bn = b_dims[-1][0]
    tmp = [0] * am
    _dot_into(pp.a[-1], t[off:off + an], tmp, 0)
    for i in range(bn):
        t[off + an + i] = _horner(tmp, i + 1)
    out_off = off + an + bn
    in_off = off + an + am
    for k in reversed(range(len(a_dims))):
        in_off -= a_dims[k][1]
        n, m, _ = b_dims[k]
        _dot_into(pp.b[k], t[in_off:in_off + n], t, out_off)
        out_off += m
    assert in_off == a_dims[0][0] and out_off == pp.codeword_len
    return t


# ------------------------------------------------------------------ one state, straight-line (the transcript's sponge)
def _gen_keccak_f():
    """oracle.pyref.keccak.keccak_f written out as straight-line code over 25 locals (the same permutation, ~10x
    faster in CPython); test_brakedown_cpu.py checks it against the oracle's"""
    m = "0xFFFFFFFFFFFFFFFF"
    rol = lambda v, n: v if n == 0 else "((({v} << {n}) | ({v} >> {r})) & {m})".format(v=v, n=n, r=64 - n, m=m)
    lines = ["def keccak_f_fast(st):", "    " + ", ".join("a%d" % i for i in range(25)) + " = st",
             "    for rc in _RC:"]
    for x in range(5):
        lines.append("        c%d = a%d ^ a%d ^ a%d ^ a%d ^ a%d" % (x, x, x + 5, x + 10, x + 15, x + 20))
    for x in range(5):
        lines.append("        d%d = c%d ^ %s" % (x, (x + 4) % 5, rol("c%d" % ((x + 1) % 5), 1)))
    for x in range(5):
        for y in range(5):
            lines.append("        b%d = %s" % (y + 5 * ((2 * x + 3 * y) % 5), rol("(a%d ^ d%d)" % (x + 5 * y, x),
                                                                               _RHO[x + 5 * y])))
    for y in range(5):
        for x in range(5):
            lines.append("        a%d = b%d ^ ((b%d ^ %s) & b%d)" % (x + 5 * y, x + 5 * y, (x + 1) % 5 + 5 * y, m,
                                                                    (x + 2) % 5 + 5 * y))
    lines.append("        a0 ^= rc")
    lines.append("    return [" + ", ".join("a%d" % i for i in range(25)) + "]")
    env = {"_RC": _RC}
    exec("\n".join(lines), env)
    return env["keccak_f_fast"]


keccak_f_fast = _gen_keccak_f()


class FastKeccak256(Keccak256):
    def _absorb_block(self, block):
        for i in range(RATE // 8):
            self.state[i] ^= int.from_bytes(block[8 * i:8 * i + 8], "little")
        self.state = keccak_f_fast(self.state)


# ------------------------------------------------------------------ transcript with hash commitments
class Transcript(Keccak256Transcript):
    """Keccak256Transcript + TranscriptWrite/Read<Output<Keccak256>, Fr>: hashes are raw stream bytes, never absorbed"""

    def __init__(self, proof=None):
        super().__init__(proof)
        self.state = FastKeccak256()

    def write_hash(self, h):
        assert len(h) == 32
        self.stream += h

    def read_hash(self):
        return bytes(self._read(32))


def squeeze_challenge_idx(tr, cap):
    return (tr.squeeze_challenge() & 0xFFFFFFFF) % cap  # first 4 bytes of to_repr, LE (brakedown.rs:427-435)


def point_to_tensor(num_rows, point):
    k = num_rows.bit_length() - 1
    hi, lo = point[:len(point) - k], point[len(point) - k:]
    return eq_xy(lo), eq_xy(hi)


# ------------------------------------------------------------------ commit / open / verify
class Commitment:
    def __init__(self, rows, hashes):
        self.rows, self.hashes = rows, hashes  # rows: num_rows lists of codeword_len; hashes: (2 << depth) - 1 bytes
        self.root = hashes[-1]


def column_hash(items):
    h = FastKeccak256()
    for x in items:
        h.update(to_repr_le(x))
    return h.finalize_reset()


def commit(pp, evals):
    assert len(evals) == 1 << pp.num_vars
    rows = [encode(pp, evals[r * pp.row_len:(r + 1) * pp.row_len]) for r in range(pp.num_rows)]
    width = 1 << pp.depth
    words = np.zeros((pp.codeword_len, 4 * pp.num_rows), dtype=np.uint64)
    for r, row in enumerate(rows):
        for c, x in enumerate(row):
            for j in range(4):
                words[c, 4 * r + j] = (x >> (64 * j)) & 0xFFFFFFFFFFFFFFFF
    level = np.zeros((width, 4), dtype=np.uint64)
    level[:pp.codeword_len] = keccak256_words(words)
    hashes = digests_to_bytes(level)
    while width > 1:
        level = keccak256_words(level.reshape(width // 2, 8))
        hashes += digests_to_bytes(level)
        width //= 2
    assert len(hashes) == (2 << pp.depth) - 1
    return Commitment(rows, hashes)


def open_(pp, evals, comm, point, tr):
    row_len, num_rows = pp.row_len, pp.num_rows
    t_0, _ = point_to_tensor(num_rows, point)

    def combine(coeffs):
        return [sum(coeffs[r] * evals[r * row_len + c] for r in range(num_rows)) % P for c in range(row_len)]

    if num_rows > 1:
        for _ in range(pp.num_proximity_testing):
            tr.write_field_elements(combine(tr.squeeze_challenges(num_rows)))
        tr.write_field_elements(combine(t_0))
    else:
        tr.write_field_elements(evals)
    for _ in range(pp.num_column_opening):
        column = squeeze_challenge_idx(tr, pp.codeword_len)
        tr.write_field_elements([comm.rows[r][column] for r in range(num_rows)])
        offset = 0
        for idx in range(pp.depth):
            tr.write_hash(comm.hashes[offset + ((column >> idx) ^ 1)])
            offset += 1 << (pp.depth - idx)


def read_commitments(num, tr):
    return [tr.read_hash() for _ in range(num)]


def verify(vp, root, point, value, tr):
    """pcs/multilinear/brakedown.rs:315-396; raises PcsError with the reference's strings"""
    row_len, num_rows = vp.row_len, vp.num_rows
    t_0, t_1 = point_to_tensor(num_rows, point)
    combined = []
    if num_rows > 1:
        coeffs = tr.squeeze_challenges(num_rows)
        combined.append((coeffs, encode(vp, tr.read_field_elements(row_len))))
    combined.append((t_0, encode(vp, tr.read_field_elements(row_len))))
    for _ in range(vp.num_column_opening):
        column = squeeze_challenge_idx(tr, vp.codeword_len)
        items = tr.read_field_elements(num_rows)
        path = [tr.read_hash() for _ in range(vp.depth)]
        for coeffs, enc in combined:
            item = sum(c * x for c, x in zip(coeffs, items)) % P if num_rows > 1 else items[0]
            if item != enc[column]:
                raise PcsError("Proximity failure")
        out = column_hash(items)
        for idx, sib in enumerate(path):
            h = FastKeccak256()
            h.update(out + sib if (column >> idx) & 1 == 0 else sib + out)
            out = h.finalize_reset()
        if out != root:
            raise PcsError("Invalid merkle tree opening")
    if sum(a * b for a, b in zip(combined[-1][1][:row_len], t_1)) % P != value % P:
        raise PcsError("Consistency failure")


__all__ = ["Params", "Spec", "commit", "open_", "verify", "read_commitments", "encode", "Transcript", "PcsError",
           "TranscriptError", "SPECS", "LOG2_Q", "point_to_tensor", "squeeze_challenge_idx", "keccak256_words"]
