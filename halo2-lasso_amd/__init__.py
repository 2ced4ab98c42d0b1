"""halo2-lasso_amd: MI355X-native prover hot path of DoHoonKim8/halo2-lasso.

Host-side mirror (Python, over the C-ABI in include/lasso_hip.h) of the reference's interface for
the path: names and argument meaning follow plonkish_backend --
  util::transcript::Keccak256Transcript, poly::multilinear::MultilinearPolynomial,
  piop::sum_check::{ClassicSumCheck, EvaluationsProver, CoefficientsProver},
  piop::gkr::prove_fractional_sum_check, util::arithmetic::variable_base_msm,
  pcs::multilinear::MultilinearKzg, and the Lasso prover (no reference code).
All compute happens in liblasso_hip.so on the GPU; this module only marshals.
"""
import ctypes as C

from . import _ffi
from ._ffi import (lh_fr, lh_g1, lh_sop, lh_evaluation, lh_lasso_table, lh_transcript,
                   LH_SC_EVALUATIONS, LH_SC_COEFFICIENTS)

R_MOD = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
Q_MOD = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
_MONT = 1 << 256
_MONT_INV_R = pow(_MONT, -1, R_MOD)
_MONT_INV_Q = pow(_MONT, -1, Q_MOD)

SUBTABLE_IDENTITY, SUBTABLE_AND, SUBTABLE_XOR = 0, 1, 2
SUBTABLE_OR, SUBTABLE_EQ, SUBTABLE_LTU = 3, 4, 5  # x | y; (x == y); (x < y) unsigned - index x || y as for AND and XOR


# ------------------------------------------------------------------ errors (plonkish_backend/src/lib.rs:12-20)
class Error(Exception):
    code = None


class InvalidSumcheck(Error):
    code = _ffi.LH_ERR_INVALID_SUMCHECK


class InvalidPcsParam(Error):
    code = _ffi.LH_ERR_INVALID_PCS_PARAM


class InvalidPcsOpen(Error):
    code = _ffi.LH_ERR_INVALID_PCS_OPEN


class InvalidSnark(Error):
    code = _ffi.LH_ERR_INVALID_SNARK


class Serialization(Error):
    code = _ffi.LH_ERR_SERIALIZATION


class TranscriptError(Error):
    code = _ffi.LH_ERR_TRANSCRIPT


class DeviceError(Error):
    code = _ffi.LH_ERR_DEVICE


class ArgumentError(Error):  # an assert!/panic in the reference
    code = _ffi.LH_ERR_ARG


_ERRORS = {e.code: e for e in (InvalidSumcheck, InvalidPcsParam, InvalidPcsOpen, InvalidSnark,
                               Serialization, TranscriptError, DeviceError, ArgumentError)}


def _check(rc):
    if rc != 0:
        msg = _ffi.load().lh_last_error()
        raise _ERRORS.get(rc, Error)((msg or b"").decode() or "lh_status %d" % rc)


# ------------------------------------------------------------------ marshalling
def fr_to_bytes(x):
    """Python int -> 32 bytes of a Montgomery `bn256::Fr`."""
    return (x % R_MOD * _MONT % R_MOD).to_bytes(32, "little")


def fr_from_bytes(b):
    return int.from_bytes(bytes(b), "little") * _MONT_INV_R % R_MOD


def frs_to_bytes(xs):
    return b"".join(fr_to_bytes(x) for x in xs)


def frs_from_bytes(b):
    return [fr_from_bytes(b[i:i + 32]) for i in range(0, len(b), 32)]


def g1_to_bytes(pt):
    """(x, y) ints or None (identity = (0,0)) -> 64 bytes of a Montgomery `bn256::G1Affine`."""
    if pt is None:
        return bytes(64)
    return b"".join((v % Q_MOD * _MONT % Q_MOD).to_bytes(32, "little") for v in pt)


def g1_from_bytes(b):
    b = bytes(b)
    x = int.from_bytes(b[:32], "little") * _MONT_INV_Q % Q_MOD
    y = int.from_bytes(b[32:], "little") * _MONT_INV_Q % Q_MOD
    return None if x == 0 and y == 0 else (x, y)


def g2_to_bytes(pt):
    """((x0, x1), (y0, y1)) or None -> 128 bytes of a Montgomery `bn256::G2Affine` (x.c0 | x.c1 | y.c0 | y.c1)."""
    if pt is None:
        return bytes(128)
    return b"".join((v % Q_MOD * _MONT % Q_MOD).to_bytes(32, "little") for c in pt for v in c)


def g2_from_bytes(b):
    b = bytes(b)
    v = [int.from_bytes(b[32 * i:32 * i + 32], "little") * _MONT_INV_Q % Q_MOD for i in range(4)]
    return None if not any(v) else ((v[0], v[1]), (v[2], v[3]))


def _fr_array(xs):
    arr = (lh_fr * max(len(xs), 1))()
    C.memmove(arr, frs_to_bytes(xs), 32 * len(xs))
    return arr


def _fr_list(arr, n):
    return frs_from_bytes(C.string_at(arr, 32 * n))


# ------------------------------------------------------------------ context / device memory
def parse_cpulist(text):
    """the kernel's CPU list format ("0-63,128-191") as a set"""
    out = set()
    for part in text.strip().split(","):
        if not part:
            continue
        lo, _, hi = part.partition("-")
        out.update(range(int(lo), int(hi or lo) + 1))
    return out


class Context:
    """One per process per GPU (`lh_ctx`)."""

    def __init__(self, device_id=0):
        self.lib = _ffi.load()
        h = C.c_void_p()
        _check(self.lib.lh_ctx_create(device_id, C.byref(h)))
        self.h = h

    def close(self):
        if self.h:
            self.lib.lh_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        _check(self.lib.lh_ctx_sync(self.h))

    def compute_units(self):
        """the compute units of the ctx's device (lh_ctx_compute_units)"""
        n = C.c_size_t()
        _check(self.lib.lh_ctx_compute_units(self.h, C.byref(n)))
        return n.value

    def host_cpus(self):
        """(PCI address of the ctx's device, the CPUs on its NUMA node as a set) - lh_ctx_host_cpus; the set is empty where
        the system does not say"""
        bus, cpus = C.create_string_buffer(64), C.create_string_buffer(4096)
        _check(self.lib.lh_ctx_host_cpus(self.h, bus, 64, cpus, 4096))
        return bus.value.decode(), parse_cpulist(cpus.value.decode())

    def bind_host(self):
        """Bind the CALLING thread to the CPUs next to the ctx's device - what a one-process-per-GPU deployment does with
        numactl.  Threads the library starts AFTERWARDS from this thread inherit the mask (its host pool, which also sizes
        itself by the mask; the helper ctx's worker); threads that exist already keep theirs, and threads created while
        bound stay bound when the caller restores its own mask: call this BEFORE the first proof of the process.  Returns
        the previous affinity mask (give it to os.sched_setaffinity to undo), or None when nothing was changed: no such
        list, or none of its CPUs is in the present mask."""
        import os
        _, local = self.host_cpus()
        before = os.sched_getaffinity(0)
        want = local & before
        if not want or want == before:
            return None
        os.sched_setaffinity(0, want)
        return before

    @property
    def stream(self):
        return self.lib.lh_ctx_stream(self.h)

    def alloc(self, nbytes):
        return DeviceBuffer(self, nbytes)

    def upload(self, data):
        buf = DeviceBuffer(self, len(data))
        buf.write(data)
        return buf


class DeviceBuffer:
    def __init__(self, ctx, nbytes, ptr=None):
        self.ctx, self.nbytes, self.owned = ctx, nbytes, ptr is None
        if ptr is None:
            p = C.c_void_p()
            _check(ctx.lib.lh_alloc(ctx.h, nbytes, C.byref(p)))
            ptr = p.value
        self.ptr = ptr

    def write(self, data, offset=0):
        data = bytes(data)
        assert offset + len(data) <= self.nbytes
        _check(self.ctx.lib.lh_upload(self.ctx.h, self.ptr + offset, data, len(data)))

    def read(self, nbytes=None, offset=0):
        nbytes = self.nbytes - offset if nbytes is None else nbytes
        out = C.create_string_buffer(nbytes)
        _check(self.ctx.lib.lh_download(self.ctx.h, out, self.ptr + offset, nbytes))
        return out.raw

    def free(self):
        if self.owned and self.ptr and self.ctx.h:
            self.ctx.lib.lh_free(self.ctx.h, self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _ptr_array(bufs):
    arr = (C.c_void_p * max(len(bufs), 1))()
    for i, b in enumerate(bufs):
        arr[i] = b.ptr if hasattr(b, "ptr") else b
    return arr


# ------------------------------------------------------------------ transcript
class Keccak256Transcript:
    """util::transcript::Keccak256Transcript<Cursor<Vec<u8>>> living in the library: `Keccak256Transcript()`
    writes (InMemoryTranscript::new), `Keccak256Transcript.from_proof(bytes)` reads (transcript.rs:110-123)."""

    def __init__(self, proof=None):
        self.lib = _ffi.load()
        p = C.POINTER(lh_transcript)()
        if proof is None:
            _check(self.lib.lh_keccak_transcript_new(C.byref(p)))
        else:
            _check(self.lib.lh_keccak_transcript_from_proof(bytes(proof), len(proof), C.byref(p)))
        self.p = p

    @classmethod
    def from_proof(cls, proof):
        return cls(proof)

    def read_field_element(self):
        out = lh_fr()
        _check(self._vt().read_field_element(self._vt().user, C.byref(out)))
        return fr_from_bytes(bytes(out))

    def read_field_elements(self, n):
        return [self.read_field_element() for _ in range(n)]

    def read_commitment(self):
        out = lh_g1()
        _check(self._vt().read_commitment(self._vt().user, C.byref(out)))
        return g1_from_bytes(bytes(out))

    def read_commitments(self, n):
        return [self.read_commitment() for _ in range(n)]

    def remaining(self):
        n = C.c_size_t()
        _check(self.lib.lh_keccak_transcript_remaining(self.p, C.byref(n)))
        return n.value

    def _vt(self):
        return self.p.contents

    def write_field_element(self, fe):
        _check(self._vt().write_field_element(self._vt().user, C.byref(_fr_array([fe])[0])))

    def write_field_elements(self, fes):
        for fe in fes:
            self.write_field_element(fe)

    def common_field_element(self, fe):
        _check(self._vt().common_field_element(self._vt().user, C.byref(_fr_array([fe])[0])))

    def squeeze_challenge(self):
        out = lh_fr()
        _check(self._vt().squeeze_challenge(self._vt().user, C.byref(out)))
        return fr_from_bytes(bytes(out))

    def squeeze_challenges(self, n):
        return [self.squeeze_challenge() for _ in range(n)]

    def write_commitment(self, pt):
        g = lh_g1()
        C.memmove(C.byref(g), g1_to_bytes(pt), 64)
        _check(self._vt().write_commitment(self._vt().user, C.byref(g)))

    def write_commitments(self, pts):
        for pt in pts:
            self.write_commitment(pt)

    def hash_io(self):
        """the lh_hash_transcript of this transcript: TranscriptWrite/Read<Output<Keccak256>, Fr>"""
        if getattr(self, "_hio", None) is None:
            hio = _ffi.lh_hash_transcript()
            _check(self.lib.lh_keccak_transcript_hash_io(self.p, C.byref(hio)))
            self._hio = hio
        return self._hio

    def write_hash(self, h):
        """32 raw bytes into the stream, not absorbed (util/transcript.rs:259-265)"""
        h = bytes(h)
        if len(h) != 32:
            raise ArgumentError("a Keccak-256 output is 32 bytes")
        hio = self.hash_io()
        _check(hio.write_hash(hio.user, (C.c_uint8 * 32).from_buffer_copy(h)))

    def read_hash(self):
        hio, out = self.hash_io(), (C.c_uint8 * 32)()
        _check(hio.read_hash(hio.user, out))
        return bytes(out)

    def into_proof(self):
        ptr, n = C.POINTER(C.c_uint8)(), C.c_size_t()
        _check(self.lib.lh_keccak_transcript_proof(self.p, C.byref(ptr), C.byref(n)))
        return C.string_at(ptr, n.value)

    def __del__(self):
        try:
            if self.p:
                self.lib.lh_keccak_transcript_free(self.p)
                self.p = None
        except Exception:
            pass


# ------------------------------------------------------------------ poly::multilinear
class MultilinearPolynomial:
    """Device-resident evaluation table of 2^num_vars Fr (poly/multilinear.rs:20-24)."""

    def __init__(self, ctx, buf, num_vars):
        self.ctx, self.buf, self.num_vars = ctx, buf, num_vars

    @property
    def ptr(self):
        return self.buf.ptr

    def __len__(self):
        return 1 << self.num_vars

    @classmethod
    def new(cls, ctx, evals):
        n = len(evals)
        assert n and n & (n - 1) == 0
        return cls(ctx, ctx.upload(frs_to_bytes(evals)), n.bit_length() - 1)

    @classmethod
    def from_u32(cls, ctx, values):
        import array
        n = len(values)
        assert n and n & (n - 1) == 0
        src = ctx.upload(array.array("I", values).tobytes())
        out = ctx.alloc(32 * n)
        _check(ctx.lib.lh_fr_from_u32(ctx.h, src.ptr, n, out.ptr))
        ctx.sync()
        return cls(ctx, out, n.bit_length() - 1)

    @classmethod
    def eq_xy(cls, ctx, y):
        out = ctx.alloc(32 << len(y))
        _check(ctx.lib.lh_eq_xy(ctx.h, _fr_array(y), len(y), out.ptr))
        return cls(ctx, out, len(y))

    def evals(self):
        return frs_from_bytes(self.buf.read(32 << self.num_vars))

    def fix_var(self, x):
        out = self.ctx.alloc(32 << (self.num_vars - 1))
        _check(self.ctx.lib.lh_fix_var(self.ctx.h, self.ptr, 1 << self.num_vars, _fr_array([x]), out.ptr))
        return MultilinearPolynomial(self.ctx, out, self.num_vars - 1)

    def evaluate(self, x):
        return evaluate_polys(self.ctx, [self], x)[0]


def evaluate_polys(ctx, polys, x):
    out = (lh_fr * len(polys))()
    _check(ctx.lib.lh_evaluate(ctx.h, _ptr_array(polys), len(polys), len(x), _fr_array(x), out))
    return _fr_list(out, len(polys))


# ------------------------------------------------------------------ piop::sum_check
EvaluationsProver = LH_SC_EVALUATIONS
CoefficientsProver = LH_SC_COEFFICIENTS


class SumOfProducts:
    """[eq_xy(ys[global_eq]) *] sum_m coeff_m * prod_k table[id]; ids < len(polys) are polys,
    ids >= len(polys) are eq_xy(ys[id - len(polys)]) -- the Expression shapes of
    fractional_sum_check.rs:272-281 and pcs/multilinear.rs:182-190."""

    def __init__(self, terms, global_eq=-1):
        self.terms, self.global_eq = [(c % R_MOD, list(f)) for c, f in terms], global_eq

    def to_c(self):
        s = lh_sop()
        s.num_terms, s.global_eq = len(self.terms), self.global_eq
        for m, (coeff, facs) in enumerate(self.terms):
            C.memmove(C.byref(s.coeff[m]), fr_to_bytes(coeff), 32)
            s.num_factors[m] = len(facs)
            for k, f in enumerate(facs):
                s.factor[m][k] = f
        return s


class ClassicSumCheck:
    @staticmethod
    def prove(ctx, prover, num_vars, expression, polys, ys, sum_, transcript):
        """ClassicSumCheck::<P>::prove (classic.rs:208-240) -> (challenges, evals)."""
        if len(expression.terms) > _ffi.LH_SC_MAX_TERMS:
            raise ArgumentError("too many terms")
        ys_flat = [v for y in ys for v in y]
        ch = (lh_fr * max(num_vars, 1))()
        ev = (lh_fr * max(len(polys), 1))()
        sop = expression.to_c()
        _check(ctx.lib.lh_sumcheck_prove(ctx.h, prover, num_vars, C.byref(sop), _ptr_array(polys), len(polys),
                                         _fr_array(ys_flat), len(ys), _fr_array([sum_]), transcript.p, ch, ev))
        return _fr_list(ch, num_vars), _fr_list(ev, len(polys))


def sum_check_prove_expression(ctx, num_vars, expression, polys, challenges, ys, sum_, transcript):
    """ClassicSumCheck::<EvaluationsProver>::prove over VirtualPolynomial{expression, polys, challenges, ys}
    (piop/sum_check.rs:16-37, classic.rs:208-240) for a general `expression.Expression`
    (rotations, Identity, Lagrange) -> (challenges x, evals of every poly at x)."""
    ce, keep = expression.to_c()
    ys_flat = [v for y in ys for v in y]
    ch = (lh_fr * max(num_vars, 1))()
    ev = (lh_fr * max(len(polys), 1))()
    _check(ctx.lib.lh_sumcheck_prove_expr(ctx.h, num_vars, C.byref(ce), _ptr_array(polys), len(polys),
                                          _fr_array(challenges), len(challenges), _fr_array(ys_flat), len(ys),
                                          _fr_array([sum_]), transcript.p, ch, ev))
    return _fr_list(ch, num_vars), _fr_list(ev, len(polys))


# ------------------------------------------------------------------ piop::gkr
def prove_fractional_sum_check(ctx, claimed_p_0s, claimed_q_0s, ps, qs, transcript):
    """fractional_sum_check.rs:89-190 -> (p_xs, q_xs, x)."""
    B = len(ps)
    if not (B == len(qs) == len(claimed_p_0s) == len(claimed_q_0s)):
        raise ArgumentError("length mismatch")  # :105-107 assert_eq
    num_vars = ps[0].num_vars if B else 0
    for p in list(ps) + list(qs):
        if p.num_vars != num_vars:
            raise ArgumentError("num_vars mismatch")  # :108-110

    def opt(claims):
        keep = [_fr_array([c]) if c is not None else None for c in claims]
        arr = (C.POINTER(lh_fr) * max(B, 1))()
        for i, k in enumerate(keep):
            arr[i] = C.cast(k, C.POINTER(lh_fr)) if k is not None else None
        return arr, keep

    cp, keep_p = opt(claimed_p_0s)
    cq, keep_q = opt(claimed_q_0s)
    p_xs, q_xs, x = (lh_fr * max(B, 1))(), (lh_fr * max(B, 1))(), (lh_fr * max(num_vars, 1))()
    _check(ctx.lib.lh_gkr_fractional_prove(ctx.h, B, num_vars, cp, cq, _ptr_array(ps), _ptr_array(qs),
                                           transcript.p, p_xs, q_xs, x))
    return _fr_list(p_xs, B), _fr_list(q_xs, B), _fr_list(x, num_vars)


def prove_grand_product(ctx, leaves, transcript):
    """Batched product-tree GKR (Lasso memory check) -> (roots, [(claim, point)])."""
    B = len(leaves)
    nv = (C.c_size_t * max(B, 1))(*[p.num_vars for p in leaves])
    total = sum(p.num_vars for p in leaves)
    roots, claims, points = (lh_fr * max(B, 1))(), (lh_fr * max(B, 1))(), (lh_fr * max(total, 1))()
    _check(ctx.lib.lh_grand_product_prove(ctx.h, B, _ptr_array(leaves), nv, transcript.p, roots, claims, points))
    pts, flat, off = [], _fr_list(points, total), 0
    for p in leaves:
        pts.append(flat[off:off + p.num_vars])
        off += p.num_vars
    return _fr_list(roots, B), list(zip(_fr_list(claims, B), pts))


# ------------------------------------------------------------------ util::arithmetic::msm
def variable_base_msm(ctx, scalars, bases, n=None):
    """msm.rs:84-181 on device buffers -> affine (x, y) ints or None for the identity."""
    n = len(scalars) if n is None else n
    out = lh_g1()
    _check(ctx.lib.lh_msm(ctx.h, scalars.ptr, bases.ptr, n, C.byref(out)))
    return g1_from_bytes(bytes(out))


def variable_base_msm_u32(ctx, scalars, bases, n):
    out = lh_g1()
    _check(ctx.lib.lh_msm_u32(ctx.h, scalars.ptr, bases.ptr, n, C.byref(out)))
    return g1_from_bytes(bytes(out))


# ------------------------------------------------------------------ pcs::multilinear::kzg
class Evaluation:
    """pcs.rs:132-155"""

    def __init__(self, poly, point, value):
        self.poly, self.point, self.value = poly, point, value % R_MOD


class _PointPcs:
    """What the schemes whose commitments are G1 points share.  A scheme NAME has the entries lh_<NAME>_batch_commit / open /
    batch_open(ctx, *pp.head(), ...) and lh_<NAME>_verify / batch_verify(*vp.head(), ...): a param says how it crosses the
    boundary through head(), and names its lh_lasso_* / lh_hyperplonk_* entries through `suffix`."""
    NAME = None

    @staticmethod
    def _chunks(pp):
        """points per commitment where a commitment is a list of points (HyraxParam.num_chunks); None: it is one point"""
        return getattr(pp, "num_chunks", None)

    @staticmethod
    def _points(vp, comms):
        return list(comms) if _PointPcs._chunks(vp) is None else [p for cm in comms for p in cm]

    @classmethod
    def _fn(cls, what):
        return getattr(_ffi.load(), "lh_%s_%s" % (cls.NAME, what))

    @classmethod
    def batch_commit(cls, pp, polys):
        if not polys:
            return []
        k = cls._chunks(pp)
        n = len(polys) * (k or 1)
        out = (lh_g1 * n)()
        _check(cls._fn("batch_commit")(pp.ctx.h, *pp.head(), _ptr_array(polys), len(polys), polys[0].num_vars, out))
        raw = C.string_at(out, 64 * n)
        pts = [g1_from_bytes(raw[64 * i:64 * i + 64]) for i in range(n)]
        return pts if k is None else [pts[i * k:(i + 1) * k] for i in range(len(polys))]

    @classmethod
    def commit(cls, pp, poly):
        return cls.batch_commit(pp, [poly])[0]

    @classmethod
    def batch_commit_and_write(cls, pp, polys, transcript):
        comms = cls.batch_commit(pp, polys)
        for comm in [comms] if cls._chunks(pp) is None else comms:
            transcript.write_commitments(comm)
        return comms

    @classmethod
    def open(cls, pp, poly, point, transcript):
        _check(cls._fn("open")(pp.ctx.h, *pp.head(), poly.ptr, poly.num_vars, _fr_array(point), transcript.p))

    @classmethod
    def batch_open(cls, pp, num_vars, polys, points, evals, transcript):
        for p in points:
            if len(p) != num_vars:
                raise InvalidPcsParam("Invalid point (expect point to have %d variates but got %d)" % (num_vars, len(p)))
        flat = [v for p in points for v in p]
        _check(cls._fn("batch_open")(pp.ctx.h, *pp.head(), num_vars, _ptr_array(polys), len(polys), _fr_array(flat),
                                     len(points), _evaluations(evals), len(evals), transcript.p))

    @classmethod
    def verify(cls, vp, comm, point, eval_, transcript):
        _check(cls._fn("verify")(*vp.head(), _g1_array(cls._points(vp, [comm])), _fr_array(point), len(point),
                                 _fr_array([eval_]), transcript.p))

    @classmethod
    def batch_verify(cls, vp, num_vars, comms, points, evals, transcript):
        flat = [v for p in points for v in p]
        _check(cls._fn("batch_verify")(*vp.head(), num_vars, _g1_array(cls._points(vp, comms)), len(comms), _fr_array(flat),
                                       len(points), _evaluations(evals), len(evals), transcript.p))


class MultilinearKzgParams:
    suffix = ""  # of the lh_lasso_* / lh_hyperplonk_* entries over this scheme

    def __init__(self, ctx, handle, borrowed=False):
        self.ctx, self.h, self.borrowed = ctx, handle, borrowed

    def view(self, ctx):
        """The same SRS (device memory, owned by this object - keep it alive) for use through another ctx of the same
        device: a second proof in flight on its own stream (bench.py two_proofs_in_flight / sharded_two_in_flight)."""
        return MultilinearKzgParams(ctx, self.h, borrowed=True)

    def head(self):
        return (self.h,)

    @property
    def num_vars(self):
        return self.ctx.lib.lh_srs_num_vars(self.h)

    def eqs_bytes(self):
        """the flat SRS as the device holds it: level k (2^k points of 64 bytes) at offset 2^k - 1"""
        total = (2 << self.num_vars) - 1
        out = C.create_string_buffer(64 * total)
        _check(self.ctx.lib.lh_srs_download(self.ctx.h, self.h, out))
        return out.raw

    def eqs(self):
        """All levels as lists of affine points (level k has 2^k)."""
        n = self.num_vars
        total = (2 << n) - 1
        out = C.create_string_buffer(64 * total)
        _check(self.ctx.lib.lh_srs_download(self.ctx.h, self.h, out))
        pts = [g1_from_bytes(out.raw[64 * i:64 * i + 64]) for i in range(total)]
        return [pts[(1 << k) - 1:(2 << k) - 1] for k in range(n + 1)]

    def free(self):
        if self.h and self.ctx.h and not self.borrowed:
            self.ctx.lib.lh_srs_free(self.ctx.h, self.h)
        self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class MultilinearKzg(_PointPcs):
    """pcs/multilinear/kzg.rs:150-361 (prover side)."""
    NAME = "mkzg"

    @staticmethod
    def setup(ctx, ss):
        """kzg.rs:166-228 with the trapdoor `ss` explicit."""
        h = C.c_void_p()
        _check(ctx.lib.lh_mkzg_setup(ctx.h, _fr_array(ss), len(ss), C.byref(h)))
        return MultilinearKzgParams(ctx, h)

    @staticmethod
    def upload(ctx, eqs_levels):
        flat = b"".join(g1_to_bytes(p) for lvl in eqs_levels for p in lvl)
        return MultilinearKzg.upload_bytes(ctx, flat, len(eqs_levels) - 1)

    @staticmethod
    def upload_bytes(ctx, eqs_flat, num_vars):
        """eqs_flat: (2^(num_vars+1) - 1) * 64 bytes in the device layout (e.g. from params_io.read_*)"""
        if len(eqs_flat) != 64 * ((2 << num_vars) - 1):
            raise ArgumentError("flat SRS has the wrong length")
        h = C.c_void_p()
        _check(ctx.lib.lh_srs_upload(ctx.h, eqs_flat, num_vars, C.byref(h)))
        return MultilinearKzgParams(ctx, h)

    @staticmethod
    def commit(pp, poly):
        out = lh_g1()
        _check(pp.ctx.lib.lh_mkzg_commit(pp.ctx.h, pp.h, poly.ptr, poly.num_vars, C.byref(out)))
        return g1_from_bytes(bytes(out))

    verify = staticmethod(lambda vp, comm, point, eval_, transcript: mkzg_verify(vp, comm, point, eval_, transcript))
    batch_verify = staticmethod(lambda vp, num_vars, comms, points, evals, transcript:
                                mkzg_batch_verify(vp, num_vars, comms, points, evals, transcript))

    @staticmethod
    def open(pp, poly, point, transcript):
        out = lh_fr()
        _check(pp.ctx.lib.lh_mkzg_open(pp.ctx.h, pp.h, poly.ptr, poly.num_vars, _fr_array(point), transcript.p,
                                       C.byref(out)))
        return fr_from_bytes(bytes(out))


class MultilinearKzgVerifierParams:
    """MultilinearKzgVerifierParams (kzg.rs:79-101): g1, g2, ss[i] = s_i * g2.  Host only."""
    suffix = ""

    def __init__(self, handle):
        self.lib, self.h = _ffi.load(), handle

    @classmethod
    def setup(cls, ss):
        """the verifier half of MultilinearKzg.setup for the same trapdoor"""
        h = C.c_void_p()
        _check(_ffi.load().lh_mkzg_vp_setup(_fr_array(ss), len(ss), C.byref(h)))
        return cls(h)

    @classmethod
    def new(cls, g1, g2, ss):
        h = C.c_void_p()
        a, b = _ffi.lh_g1(), _ffi.lh_g2()
        C.memmove(C.byref(a), g1_to_bytes(g1), 64)
        C.memmove(C.byref(b), g2_to_bytes(g2), 128)
        arr = (_ffi.lh_g2 * max(len(ss), 1))()
        C.memmove(arr, b"".join(g2_to_bytes(p) for p in ss), 128 * len(ss))
        _check(_ffi.load().lh_mkzg_vp_new(C.byref(a), C.byref(b), arr, len(ss), C.byref(h)))
        return cls(h)

    def head(self):
        return (self.h,)

    @property
    def num_vars(self):
        return self.lib.lh_mkzg_vp_num_vars(self.h)

    def export(self):
        """-> (g1, g2, [ss_i])"""
        n = self.num_vars
        a, b, arr = _ffi.lh_g1(), _ffi.lh_g2(), (_ffi.lh_g2 * max(n, 1))()
        _check(self.lib.lh_mkzg_vp_export(self.h, C.byref(a), C.byref(b), arr))
        raw = C.string_at(arr, 128 * n)
        return g1_from_bytes(bytes(a)), g2_from_bytes(bytes(b)), [g2_from_bytes(raw[128 * i:128 * i + 128]) for i in range(n)]

    def free(self):
        if self.h:
            self.lib.lh_mkzg_vp_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def pairings_product_is_identity(pairs):
    """util/arithmetic.rs:24-33: pairs of (G1 affine, G2 affine)"""
    n = len(pairs)
    ps, qs = (_ffi.lh_g1 * max(n, 1))(), (_ffi.lh_g2 * max(n, 1))()
    C.memmove(ps, b"".join(g1_to_bytes(p) for p, _ in pairs), 64 * n)
    C.memmove(qs, b"".join(g2_to_bytes(q) for _, q in pairs), 128 * n)
    out = C.c_int()
    _check(_ffi.load().lh_pairing_check(ps, qs, n, C.byref(out)))
    return bool(out.value)


def _evaluations(evals):
    evs = (lh_evaluation * max(len(evals), 1))()
    for i, e in enumerate(evals):
        evs[i].poly, evs[i].point = e.poly, e.point
        C.memmove(C.byref(evs[i].value), fr_to_bytes(e.value), 32)
    return evs


def _g1_array(pts):
    arr = (lh_g1 * max(len(pts), 1))()
    C.memmove(arr, b"".join(g1_to_bytes(p) for p in pts), 64 * len(pts))
    return arr


def mkzg_verify(vp, comm, point, eval_, transcript):
    """MultilinearKzg::verify (kzg.rs:330-361); raises InvalidPcsOpen"""
    _check(vp.lib.lh_mkzg_verify(vp.h, _g1_array([comm]), _fr_array(point), len(point), _fr_array([eval_]), transcript.p))


def mkzg_batch_verify(vp, num_vars, comms, points, evals, transcript):
    """additive::batch_verify (pcs/multilinear.rs:237-276)"""
    for p in points:
        if len(p) != num_vars:
            raise InvalidPcsParam("Invalid point (expect point to have %d variates but got %d)" % (num_vars, len(p)))
    flat = [v for p in points for v in p]
    _check(vp.lib.lh_mkzg_batch_verify(vp.h, num_vars, _g1_array(comms), len(comms), _fr_array(flat), len(points),
                                       _evaluations(evals), len(evals), transcript.p))


def _tail(param, transcript):
    """the arguments a scheme's Lasso entries take behind the transcript (BrakedownParam.tail); most take none"""
    tail = getattr(param, "tail", None)
    return tail(transcript) if tail else ()


def sum_check_verify(prover, num_vars, degree, sum_, transcript):
    """ClassicSumCheck::<P>::verify (classic.rs:242-272) -> (final claim, challenges)"""
    ev, ch = lh_fr(), (lh_fr * max(num_vars, 1))()
    _check(_ffi.load().lh_sumcheck_verify(prover, num_vars, degree, _fr_array([sum_]), transcript.p, C.byref(ev), ch))
    return fr_from_bytes(bytes(ev)), _fr_list(ch, num_vars)


def lasso_verify(vp, table, num_vars, transcript):
    """Verifier of the Lasso argument (oracle/pyref/lasso.py:219-261).  A Keccak256Transcript must be fully consumed."""
    t = table.to_c()
    _check(getattr(vp.lib, "lh_lasso_verify" + vp.suffix)(*vp.head(), C.byref(t), num_vars, transcript.p,
                                                          *_tail(vp, transcript)))
    if isinstance(transcript, Keccak256Transcript) and transcript.remaining():
        raise InvalidSnark("trailing bytes in proof")


def lasso_verify_batch(vp, tables, num_vars, transcript):
    """Verifier of lasso_prove_batch (tests/lasso_batch_ref.py verify).  A Keccak256Transcript must be fully consumed."""
    arr, keep = _table_list(tables)
    _check(vp.lib.lh_lasso_verify_batch(vp.h, arr, len(tables), num_vars, transcript.p))
    del keep
    if isinstance(transcript, Keccak256Transcript) and transcript.remaining():
        raise InvalidSnark("trailing bytes in proof")


# ------------------------------------------------------------------ pcs::multilinear::zeromorph over pcs::univariate::kzg
class UnivariateKzgParams:
    """UnivariateKzgParam (pcs/univariate/kzg.rs:38-66): powers_of_s_g1 resident on the device"""

    def __init__(self, ctx, handle):
        self.ctx, self.h = ctx, handle

    @property
    def size(self):
        return self.ctx.lib.lh_usrs_size(self.h)

    def powers(self):
        n = self.size
        out = C.create_string_buffer(64 * n)
        _check(self.ctx.lib.lh_usrs_download(self.ctx.h, self.h, out))
        return [g1_from_bytes(out.raw[64 * i:64 * i + 64]) for i in range(n)]

    def free(self):
        if self.h and self.ctx.h:
            self.ctx.lib.lh_usrs_free(self.ctx.h, self.h)
        self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class ZeromorphProverParam:
    """ZeromorphKzgProverParam (zeromorph.rs:29-40) = the device SRS + the trim size"""
    suffix = "_zeromorph"

    def __init__(self, params, poly_size):
        self.params, self.poly_size, self.ctx = params, poly_size, params.ctx

    def head(self):
        return (self.params.h, self.poly_size)


class ZeromorphVerifierParam:
    """ZeromorphKzgVerifierParam (zeromorph.rs:42-65), host only"""
    suffix = "_zeromorph"

    def __init__(self, handle):
        self.lib, self.h = _ffi.load(), handle

    def head(self):
        return (self.h,)

    @classmethod
    def setup(cls, s, param_size, poly_size):
        h = C.c_void_p()
        _check(_ffi.load().lh_zeromorph_vp_setup(_fr_array([s]), param_size, poly_size, C.byref(h)))
        return cls(h)

    @classmethod
    def new(cls, g1, g2, s_g2, s_offset_g2):
        h, a = C.c_void_p(), _ffi.lh_g1()
        C.memmove(C.byref(a), g1_to_bytes(g1), 64)
        gs = []
        for p in (g2, s_g2, s_offset_g2):
            b = _ffi.lh_g2()
            C.memmove(C.byref(b), g2_to_bytes(p), 128)
            gs.append(b)
        _check(_ffi.load().lh_zeromorph_vp_new(C.byref(a), C.byref(gs[0]), C.byref(gs[1]), C.byref(gs[2]), C.byref(h)))
        return cls(h)

    def export(self):
        a, b, c_, d = _ffi.lh_g1(), _ffi.lh_g2(), _ffi.lh_g2(), _ffi.lh_g2()
        _check(self.lib.lh_zeromorph_vp_export(self.h, C.byref(a), C.byref(b), C.byref(c_), C.byref(d)))
        return g1_from_bytes(bytes(a)), g2_from_bytes(bytes(b)), g2_from_bytes(bytes(c_)), g2_from_bytes(bytes(d))

    def free(self):
        if self.h:
            self.lib.lh_zeromorph_vp_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Zeromorph(_PointPcs):
    """Zeromorph<UnivariateKzg<Bn256>> (pcs/multilinear/zeromorph.rs:67-256)"""
    NAME = "zeromorph"

    @staticmethod
    def setup(ctx, s, poly_size):
        """UnivariateKzg::setup (univariate/kzg.rs:175-218) with the trapdoor explicit"""
        h = C.c_void_p()
        _check(ctx.lib.lh_ukzg_setup(ctx.h, _fr_array([s]), poly_size, C.byref(h)))
        return UnivariateKzgParams(ctx, h)

    @staticmethod
    def upload(ctx, powers):
        h = C.c_void_p()
        _check(ctx.lib.lh_usrs_upload(ctx.h, b"".join(g1_to_bytes(p) for p in powers), len(powers), C.byref(h)))
        return UnivariateKzgParams(ctx, h)

    @staticmethod
    def trim(params, poly_size):
        """zeromorph.rs:90-108 (prover half)"""
        if params.size < poly_size:
            raise InvalidPcsParam("Too large poly_size to trim to (param supports poly_size up to %d but got %d)"
                                  % (params.size, poly_size))
        return ZeromorphProverParam(params, poly_size)


# ------------------------------------------------------------------ pcs::univariate::kzg on its own, pcs::multilinear::gemini over it
class UnivariatePolynomial:
    """UnivariatePolynomial in the coefficient basis: `len` coefficients in a device buffer (fixed length: leading zero
    coefficients are kept, they change no commitment)"""

    def __init__(self, ctx, buf, length):
        self.ctx, self.buf, self.len = ctx, buf, length

    @classmethod
    def from_ints(cls, ctx, coeffs):
        return cls(ctx, ctx.upload(frs_to_bytes(coeffs)) if coeffs else None, len(coeffs))

    @property
    def ptr(self):
        return self.buf.ptr if self.buf is not None else None


class UnivariateKzgProverParam:
    """UnivariateKzgProverParam (univariate/kzg.rs:68-88) = the device SRS + the trim size"""

    def __init__(self, params, poly_size):
        self.params, self.poly_size, self.ctx = params, poly_size, params.ctx


class UnivariateKzgVerifierParam:
    """UnivariateKzgVerifierParam (univariate/kzg.rs:90-120): (g1, g2, [s]_2), host only"""

    def __init__(self, handle):
        self.lib, self.h = _ffi.load(), handle

    @classmethod
    def setup(cls, s):
        h = C.c_void_p()
        _check(_ffi.load().lh_ukzg_vp_setup(_fr_array([s]), C.byref(h)))
        return cls(h)

    @classmethod
    def new(cls, g1, g2, s_g2):
        h, a = C.c_void_p(), _ffi.lh_g1()
        C.memmove(C.byref(a), g1_to_bytes(g1), 64)
        gs = []
        for p in (g2, s_g2):
            b = _ffi.lh_g2()
            C.memmove(C.byref(b), g2_to_bytes(p), 128)
            gs.append(b)
        _check(_ffi.load().lh_ukzg_vp_new(C.byref(a), C.byref(gs[0]), C.byref(gs[1]), C.byref(h)))
        return cls(h)

    def export(self):
        a, b, c_ = _ffi.lh_g1(), _ffi.lh_g2(), _ffi.lh_g2()
        _check(self.lib.lh_ukzg_vp_export(self.h, C.byref(a), C.byref(b), C.byref(c_)))
        return g1_from_bytes(bytes(a)), g2_from_bytes(bytes(b)), g2_from_bytes(bytes(c_))

    def free(self):
        if self.h:
            self.lib.lh_ukzg_vp_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _upoly_arrays(polys):
    ptrs = (C.c_void_p * max(len(polys), 1))(*[p.ptr for p in polys])
    lens = (C.c_size_t * max(len(polys), 1))(*[p.len for p in polys])
    return ptrs, lens


class UnivariateKzg:
    """UnivariateKzg<Bn256> (pcs/univariate/kzg.rs:161-555); points are field elements"""

    setup = staticmethod(lambda ctx, s, poly_size: Zeromorph.setup(ctx, s, poly_size))
    upload = staticmethod(lambda ctx, powers: Zeromorph.upload(ctx, powers))
    PROVER_PARAM = UnivariateKzgProverParam

    @classmethod
    def trim(cls, params, poly_size):
        """kzg.rs:220-240 (prover half)"""
        if params.size < poly_size:
            raise InvalidPcsParam("Too large poly_size to trim to (param supports poly_size up to %d but got %d)"
                                  % (params.size, poly_size))
        return cls.PROVER_PARAM(params, poly_size)

    @staticmethod
    def batch_commit(pp, polys):
        if not polys:
            return []
        out = (lh_g1 * len(polys))()
        ptrs, lens = _upoly_arrays(polys)
        _check(pp.ctx.lib.lh_ukzg_batch_commit(pp.ctx.h, pp.params.h, pp.poly_size, ptrs, lens, len(polys), out))
        raw = C.string_at(out, 64 * len(polys))
        return [g1_from_bytes(raw[64 * i:64 * i + 64]) for i in range(len(polys))]

    @staticmethod
    def commit(pp, poly):
        return UnivariateKzg.batch_commit(pp, [poly])[0]

    @staticmethod
    def batch_commit_and_write(pp, polys, transcript):
        comms = UnivariateKzg.batch_commit(pp, polys)
        transcript.write_commitments(comms)
        return comms

    @staticmethod
    def open(pp, poly, point, transcript):
        _check(pp.ctx.lib.lh_ukzg_open(pp.ctx.h, pp.params.h, pp.poly_size, poly.ptr, poly.len, _fr_array([point]),
                                       transcript.p))

    @staticmethod
    def batch_open(pp, polys, points, evals, transcript):
        ptrs, lens = _upoly_arrays(polys)
        _check(pp.ctx.lib.lh_ukzg_batch_open(pp.ctx.h, pp.params.h, pp.poly_size, ptrs, lens, len(polys),
                                             _fr_array(points), len(points), _evaluations(evals), len(evals),
                                             transcript.p))

    @staticmethod
    def verify(vp, comm, point, eval_, transcript):
        _check(vp.lib.lh_ukzg_verify(vp.h, _g1_array([comm]), _fr_array([point]), _fr_array([eval_]), transcript.p))

    @staticmethod
    def batch_verify(vp, comms, points, evals, transcript):
        _check(vp.lib.lh_ukzg_batch_verify(vp.h, _g1_array(comms), len(comms), _fr_array(points), len(points),
                                           _evaluations(evals), len(evals), transcript.p))


class GeminiProverParam(UnivariateKzgProverParam):
    """Gemini's ProverParam is UnivariateKzg's (gemini.rs:36-37); a type of its own so that provers can dispatch on it"""
    suffix = "_gemini"

    def head(self):
        return (self.params.h, self.poly_size)


class GeminiVerifierParam(UnivariateKzgVerifierParam):
    """Gemini's VerifierParam is UnivariateKzg's (gemini.rs:38)"""
    suffix = "_gemini"

    def head(self):
        return (self.h,)


class Gemini(_PointPcs):
    """Gemini<UnivariateKzg<Bn256>> (pcs/multilinear/gemini.rs:29-211): the method set of Zeromorph"""
    NAME = "gemini"

    setup = staticmethod(lambda ctx, s, poly_size: Zeromorph.setup(ctx, s, poly_size))
    upload = staticmethod(lambda ctx, powers: Zeromorph.upload(ctx, powers))

    @staticmethod
    def trim(params, poly_size):
        if params.size < poly_size:
            raise InvalidPcsParam("Too large poly_size to trim to (param supports poly_size up to %d but got %d)"
                                  % (params.size, poly_size))
        return GeminiProverParam(params, poly_size)

    @staticmethod
    def folds(ctx, poly, point):
        """the folds fs[1..] of an opening at `point`, as lists of ints (tests)"""
        n = poly.num_vars
        if n < 2:
            return []
        out = ctx.alloc(32 * ((1 << n) - 2))
        _check(ctx.lib.lh_gemini_folds(ctx.h, poly.ptr, n, _fr_array(point), out.ptr))
        flat, res, off = frs_from_bytes(out.read()), [], 0
        for i in range(1, n):
            res.append(flat[off:off + (1 << (n - i))])
            off += 1 << (n - i)
        return res


# ------------------------------------------------------------------ pcs::multilinear::ipa over bn256::G1Affine
class IpaParams:
    """MultilinearIpaParams (pcs/multilinear/ipa.rs:25-44): g (2^num_vars points) and h from the library's hash-to-point
    (DESIGN.md §14).  Set up with a Context g is derived on and stays on its device (prover param); without one it is on
    the host (verifier param)."""

    def __init__(self, ctx, handle):
        self.ctx, self.lib, self.h = ctx, _ffi.load(), handle
        self.size = self.lib.lh_ipa_param_size(handle)

    def download(self):
        """-> (g, h) as affine points"""
        out, h = C.create_string_buffer(64 * self.size), lh_g1()
        _check(self.lib.lh_ipa_param_download(self.ctx.h if self.ctx is not None else None, self.h, out, C.byref(h)))
        raw = out.raw
        return [g1_from_bytes(raw[64 * i:64 * i + 64]) for i in range(self.size)], g1_from_bytes(bytes(h))

    def free(self):
        if self.h:
            self.lib.lh_ipa_param_free(self.ctx.h if self.ctx is not None else None, self.h)
        self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class IpaParam:
    """a trimmed MultilinearIpaParams (ipa.rs:129-145): the params and the trim size; prover and verifier param at once"""

    suffix = "_ipa"

    def __init__(self, params, poly_size):
        self.params, self.poly_size, self.ctx, self.lib = params, poly_size, params.ctx, params.lib

    def head(self):
        return (self.params.h, self.poly_size)


class Ipa(_PointPcs):
    """MultilinearIpa<bn256::G1Affine> (pcs/multilinear/ipa.rs:23-337): transparent and additive; the method set of Gemini"""
    NAME = "ipa"

    @staticmethod
    def setup(ctx, poly_size):
        """ipa.rs:98-127; ctx None: a host-only (verifier) param"""
        h = C.c_void_p()
        _check(_ffi.load().lh_ipa_setup(ctx.h if ctx is not None else None, poly_size, C.byref(h)))
        return IpaParams(ctx, h)

    @staticmethod
    def trim(params, poly_size):
        if poly_size < 1 or poly_size & (poly_size - 1):
            raise ArgumentError("poly_size must be a power of two")
        if params.size < poly_size:
            raise InvalidPcsParam("Too many variates to trim (param supports variates up to %d but got %d)"
                                  % (params.size.bit_length() - 1, poly_size.bit_length() - 1))
        return IpaParam(params, poly_size)

    @staticmethod
    def g1_axpy(ctx, a, b, s):
        """the base fold of a round as a primitive: [a[j] + s b[j]] for lists of affine points (None = identity)"""
        n = len(a)
        da, db = ctx.upload(b"".join(g1_to_bytes(p) for p in a)), ctx.upload(b"".join(g1_to_bytes(p) for p in b))
        out = ctx.alloc(64 * n)
        _check(ctx.lib.lh_g1_axpy(ctx.h, da.ptr, db.ptr, n, _fr_array([s]), out.ptr))
        raw = out.read()
        return [g1_from_bytes(raw[64 * i:64 * i + 64]) for i in range(n)]


class HyraxParam:
    """a trimmed MultilinearHyraxParams (hyrax.rs:26-62): the inner IPA params and the trim arguments; prover and verifier
    param at once"""

    suffix = "_hyrax"

    def __init__(self, params, poly_size, batch_size):
        self.params, self.poly_size, self.batch_size, self.ctx, self.lib = params, poly_size, batch_size, params.ctx, params.lib
        self.num_vars, self.batch_num_vars, self.row_num_vars = Hyrax.dims(poly_size, batch_size)
        self.num_chunks = 1 << (self.num_vars - self.row_num_vars)

    def head(self):
        return (self.params.h, self.poly_size, self.batch_size)


class Hyrax(_PointPcs):
    """MultilinearHyrax<bn256::G1Affine> (pcs/multilinear/hyrax.rs:23-321); a commitment is a list of num_chunks points"""
    NAME = "hyrax"

    @staticmethod
    def dims(poly_size, batch_size):
        """-> (num_vars, batch_num_vars, row_num_vars) (hyrax.rs:125-127)"""
        a, b, c_ = C.c_size_t(), C.c_size_t(), C.c_size_t()
        _check(_ffi.load().lh_hyrax_dims(poly_size, batch_size, C.byref(a), C.byref(b), C.byref(c_)))
        return a.value, b.value, c_.value

    @staticmethod
    def setup(ctx, poly_size, batch_size):
        """hyrax.rs:121-137 -> the inner IpaParams (2^row_num_vars generators); ctx None: a host-only (verifier) param"""
        h = C.c_void_p()
        _check(_ffi.load().lh_hyrax_setup(ctx.h if ctx is not None else None, poly_size, batch_size, C.byref(h)))
        return IpaParams(ctx, h)

    @staticmethod
    def trim(params, poly_size, batch_size):
        _check(params.lib.lh_hyrax_trim(params.h, poly_size, batch_size, None, None))
        return HyraxParam(params, poly_size, batch_size)

    @staticmethod
    def rows_msm(ctx, scalars_buf, n, row_len, bases_buf, u32=False, bits=0):
        """the row commitments as a primitive: [sum_c s[r row_len + c] bases[c]] for the ceil(n / row_len) rows of a device
        array of n scalars (Fr, or u32 values below 2^bits), against row_len device points (None = identity)"""
        if row_len < 1:
            raise ArgumentError("row_len must be at least 1")
        rows = (n + row_len - 1) // row_len
        out = (lh_g1 * max(rows, 1))()
        _check(ctx.lib.lh_g1_rows_msm(ctx.h, scalars_buf.ptr, 1 if u32 else 0, bits, n, row_len, bases_buf.ptr, out))
        raw = C.string_at(out, 64 * rows)
        return [g1_from_bytes(raw[64 * i:64 * i + 64]) for i in range(rows)]

    @classmethod
    def verify(cls, vp, comm, point, eval_, transcript):
        if len(comm) != vp.num_chunks:
            raise ArgumentError("expected a commitment of %d points" % vp.num_chunks)  # assert_eq! hyrax.rs:295
        super().verify(vp, comm, point, eval_, transcript)

    @classmethod
    def batch_verify(cls, vp, num_vars, comms, points, evals, transcript):
        if any(len(cm) != vp.num_chunks for cm in comms):
            raise ArgumentError("expected commitments of %d points" % vp.num_chunks)
        super().batch_verify(vp, num_vars, comms, points, evals, transcript)


# ------------------------------------------------------------------ pcs::multilinear::brakedown
class BrakedownParam:
    """MultilinearBrakedownParams (pcs/multilinear/brakedown.rs:35-41): the code's parameters and sparse matrices, drawn
    from a 32-byte seed.  Set up with a Context the matrices are also on its device (prover param);
    it is its own prover and verifier param, as in the reference."""

    suffix = "_brakedown"  # of the lh_lasso_* entries over this scheme

    def __init__(self, ctx, handle, num_vars, spec):
        self.ctx, self.h, self.num_vars, self.spec = ctx, handle, num_vars, spec
        self.lib = _ffi.load()
        v = [C.c_size_t() for _ in range(5)]
        _check(self.lib.lh_brakedown_param_info(self.h, *[C.byref(x) for x in v]))
        (self.row_len, self.num_rows, self.codeword_len, self.num_column_opening,
         self.num_proximity_testing) = [x.value for x in v]

    def info(self):
        return (self.row_len, self.num_rows, self.codeword_len, self.num_column_opening, self.num_proximity_testing)

    def head(self):
        return (self.h,)

    @staticmethod
    def tail(transcript):
        """what the entries over this scheme take behind the transcript: its hash half (roots and Merkle paths)"""
        return (C.byref(transcript.hash_io()),)

    def encode(self, msg):
        """LinearCodes::encode on the host (util/code/brakedown.rs:88-125): row_len values -> codeword_len values"""
        if len(msg) != self.row_len:
            raise ArgumentError("brakedown encode: expected %d values" % self.row_len)
        out = (lh_fr * self.codeword_len)()
        _check(self.lib.lh_brakedown_encode(self.h, _fr_array(msg), out))
        return _fr_list(out, self.codeword_len)

    def free(self):
        if self.h:
            self.lib.lh_brakedown_param_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class BrakedownVerifierParam(BrakedownParam):
    """the host-only param a verifier holds (setup without a device)"""

    @classmethod
    def derive(cls, num_vars, spec):
        """the parameters alone, without matrices: info() and trim only"""
        h = C.c_void_p()
        _check(_ffi.load().lh_brakedown_derive(num_vars, spec, C.byref(h)))
        return cls(None, h, num_vars, spec)

    @classmethod
    def setup(cls, num_vars, spec, seed):
        h = C.c_void_p()
        _check(_ffi.load().lh_brakedown_setup(None, num_vars, spec, bytes(seed), C.byref(h)))
        return cls(None, h, num_vars, spec)


class LigeroParam(BrakedownParam):
    """The param of the Ligero PCS: Brakedown's scheme with rows encoded by a systematic Reed-Solomon code of rate
    2^-log_inv_rate (tests/ligero_ref.py).  A BrakedownParam to every entry that takes one; `spec` is 0."""

    def __init__(self, ctx, handle, num_vars, log_inv_rate):
        super().__init__(ctx, handle, num_vars, 0)
        self.log_inv_rate = log_inv_rate
        self.row_vars = self.row_len.bit_length() - 1

    @classmethod
    def _make(cls, entry, ctx, num_vars, log_inv_rate, row_vars):
        if row_vars is None:
            row_vars = _ffi.LH_LIGERO_ROW_VARS_AUTO
        if not (isinstance(row_vars, int) and 0 <= row_vars <= _ffi.LH_LIGERO_ROW_VARS_AUTO):
            raise ArgumentError("ligero: row_vars must be None or a non-negative integer")
        h = C.c_void_p()
        head = () if entry == "lh_ligero_derive" else (ctx.h if ctx is not None else None,)
        _check(getattr(_ffi.load(), entry)(*head, num_vars, log_inv_rate, row_vars, C.byref(h)))
        return cls(ctx, h, num_vars, log_inv_rate)


class LigeroVerifierParam(LigeroParam):
    """the host-only param a verifier holds"""

    @classmethod
    def derive(cls, num_vars, log_inv_rate=2, row_vars=None):
        """the parameters alone, without the table of roots: info() and trim only"""
        return cls._make("lh_ligero_derive", None, num_vars, log_inv_rate, row_vars)

    @classmethod
    def setup(cls, num_vars, log_inv_rate=2, row_vars=None):
        return cls._make("lh_ligero_setup", None, num_vars, log_inv_rate, row_vars)


class Ligero:
    """Setup of the Ligero PCS; commit, open and verify are hl.Brakedown's over the returned param."""

    @staticmethod
    def setup(ctx, num_vars, log_inv_rate=2, row_vars=None):
        """row_vars None: the row length of the smallest proof"""
        return LigeroParam._make("lh_ligero_setup", ctx, num_vars, log_inv_rate, row_vars)


class BrakedownCommitment:
    """MultilinearBrakedownCommitment (brakedown.rs:55-60): the encoded rows and the Merkle tree stay on the device"""

    def __init__(self, ctx, handle):
        self.ctx, self.h, self.lib = ctx, handle, _ffi.load()
        root = C.create_string_buffer(32)
        _check(self.lib.lh_brakedown_comm_root(self.h, root))
        self.root = root.raw

    def rows(self, num_rows, codeword_len):
        out = C.create_string_buffer(32 * num_rows * codeword_len)
        _check(self.lib.lh_brakedown_comm_rows(self.ctx.h, self.h, out))
        return frs_from_bytes(out.raw)

    def rows_device_ptr(self):
        p = C.c_void_p()
        _check(self.lib.lh_brakedown_comm_rows_device(self.h, C.byref(p)))
        return p.value

    def tree(self, codeword_len):
        """the Merkle tree as raw bytes: (2 << depth) - 1 digests of 32 bytes, leaves first, the root last"""
        n = (2 << (codeword_len - 1).bit_length()) - 1
        out = C.create_string_buffer(32 * n)
        _check(self.lib.lh_brakedown_comm_tree(self.ctx.h, self.h, out))
        return out.raw

    def staged(self, pp):
        """the matrix as the staged open reads it: codeword_len x num_rows, column-major, as raw bytes"""
        out = C.create_string_buffer(32 * pp.num_rows * pp.codeword_len)
        _check(self.lib.lh_brakedown_comm_stage(self.ctx.h, pp.h, self.h, out))
        return out.raw

    def free(self):
        if self.h:
            self.lib.lh_brakedown_comm_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Brakedown:
    """MultilinearBrakedown<bn256::Fr, Keccak256, BrakedownSpec1..6> (pcs/multilinear/brakedown.rs:89-417)"""

    @staticmethod
    def setup(ctx, num_vars, spec, seed):
        """setup with poly_size = 2^num_vars; the matrices from `seed` (32 bytes) instead of an RngCore"""
        h = C.c_void_p()
        _check(_ffi.load().lh_brakedown_setup(ctx.h if ctx is not None else None, num_vars, spec, bytes(seed),
                                              C.byref(h)))
        return BrakedownParam(ctx, h, num_vars, spec)

    @staticmethod
    def trim(param, poly_size):
        """brakedown.rs:112-126: (pp, vp) = (param, param) when poly_size == 2^num_vars, else InvalidPcsParam"""
        _check(param.lib.lh_brakedown_trim(param.h, poly_size))
        return param, param

    @staticmethod
    def batch_commit(pp, polys):
        if not polys:
            return []
        out = (C.c_void_p * len(polys))()
        _check(pp.lib.lh_brakedown_batch_commit(pp.ctx.h, pp.h, _ptr_array(polys), len(polys), polys[0].num_vars, out))
        return [BrakedownCommitment(pp.ctx, C.c_void_p(out[i])) for i in range(len(polys))]

    @staticmethod
    def commit_columns(pp, cols):
        """cols: (device pointer, kind, len) per column, kind "u32" or "fr"; each committed as the table zero-padded to
        pp.num_vars variables (lh_brakedown_commit_columns)"""
        if not cols:
            return []
        n = len(cols)
        ptrs = (C.c_void_p * n)(*[p for p, _, _ in cols])
        kinds = (C.c_int * n)(*[{"fr": _ffi.LH_BD_COLUMN_FR, "u32": _ffi.LH_BD_COLUMN_U32}[k] for _, k, _ in cols])
        lens = (C.c_size_t * n)(*[ln for _, _, ln in cols])
        out = (C.c_void_p * n)()
        _check(pp.lib.lh_brakedown_commit_columns(pp.ctx.h, pp.h, ptrs, kinds, lens, n, out))
        return [BrakedownCommitment(pp.ctx, C.c_void_p(out[i])) for i in range(n)]

    @staticmethod
    def commit(pp, poly):
        out = C.c_void_p()
        _check(pp.lib.lh_brakedown_commit(pp.ctx.h, pp.h, poly.ptr, poly.num_vars, C.byref(out)))
        return BrakedownCommitment(pp.ctx, out)

    @staticmethod
    def batch_commit_and_write(pp, polys, transcript):
        """roots written as raw stream bytes, not absorbed (util/transcript.rs:259-265)"""
        comms = Brakedown.batch_commit(pp, polys)
        for c in comms:
            transcript.write_hash(c.root)
        return comms

    @staticmethod
    def open(pp, poly, comm, point, transcript):
        _check(pp.lib.lh_brakedown_open(pp.ctx.h, pp.h, poly.ptr, poly.num_vars, comm.h, _fr_array(point), transcript.p,
                                        C.byref(transcript.hash_io())))

    @staticmethod
    def batch_open(pp, num_vars, polys, comms, points, evals, transcript):
        for p in points:
            if len(p) != num_vars:
                raise InvalidPcsParam("Invalid point (expect point to have %d variates but got %d)" % (num_vars, len(p)))
        flat = [v for p in points for v in p]
        _check(pp.lib.lh_brakedown_batch_open(pp.ctx.h, pp.h, num_vars, _ptr_array(polys), _ptr_array([c.h.value for c in comms]), len(polys),
                                              _fr_array(flat), len(points), _evaluations(evals), len(evals),
                                              transcript.p, C.byref(transcript.hash_io())))

    @staticmethod
    def read_commitments(vp, num, transcript):
        out = C.create_string_buffer(32 * max(num, 1))
        _check(vp.lib.lh_brakedown_read_commitments(vp.h, num, C.byref(transcript.hash_io()), out))
        return [out.raw[32 * i:32 * i + 32] for i in range(num)]

    @staticmethod
    def verify(vp, root, point, eval_, transcript):
        _check(vp.lib.lh_brakedown_verify(vp.h, bytes(root), _fr_array(point), len(point), _fr_array([eval_]),
                                          transcript.p, C.byref(transcript.hash_io())))

    @staticmethod
    def batch_verify(vp, num_vars, roots, points, evals, transcript):
        flat = [v for p in points for v in p]
        _check(vp.lib.lh_brakedown_batch_verify(vp.h, num_vars, b"".join(bytes(r) for r in roots), len(roots),
                                                _fr_array(flat), len(points), _evaluations(evals), len(evals),
                                                transcript.p, C.byref(transcript.hash_io())))


# ------------------------------------------------------------------ Lasso
class Subtable:
    """A caller-registered subtable (lh_subtable_register): 2^chunk_bits 32-bit entries, chunk_bits <= 20.  The registry is
    process-wide and needs no Context; `kind` is what a memory of a LassoTable names (the Subtable itself does as well).
    Kinds are never reused: after close() the kind is refused.  At most LH_SUBTABLE_CUSTOM_MAX are live at a time.

        with hl.Subtable.register(sbox) as t:
            table = hl.LassoTable(1, 8, [(0, t)], [(1, [0])])
    """

    def __init__(self, kind):
        self.kind = int(kind)
        cb, vb, dg = C.c_uint32(), C.c_uint32(), C.create_string_buffer(32)
        _check(_ffi.load().lh_subtable_info(self.kind, C.byref(cb), C.byref(vb), dg))
        self.chunk_bits, self.value_bits, self.digest = cb.value, vb.value, dg.raw

    @classmethod
    def register(cls, values):
        values = [int(v) for v in values]
        n = len(values)
        if n < 2 or n & (n - 1) or n > 1 << _ffi.LH_SUBTABLE_CUSTOM_MAX_BITS:
            raise ArgumentError("subtable: 2^chunk_bits values, chunk_bits in [1, %d]" % _ffi.LH_SUBTABLE_CUSTOM_MAX_BITS)
        if any(not 0 <= v < 1 << 32 for v in values):
            raise ArgumentError("subtable: values are 32-bit unsigned")
        kind = C.c_uint32()
        _check(_ffi.load().lh_subtable_register((C.c_uint32 * n)(*values), n.bit_length() - 1, C.byref(kind)))
        return cls(kind.value)

    def close(self):
        if self.kind is not None:
            kind, self.kind = self.kind, None
            _check(_ffi.load().lh_subtable_unregister(kind))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __int__(self):
        if self.kind is None:
            raise ArgumentError("subtable: closed")
        return self.kind

    __index__ = __int__


_LTS_SUBTABLES = {}  # chunk_bits -> the signed top-chunk subtable of less_than_signed, registered once per process


class LassoTable:
    """Decomposable table: c chunks of l bits, memories (chunk, subtable), g = sum coeff * prod E_i.  A memory's subtable
    is a SUBTABLE_* kind, a Subtable, or the kind of one."""

    def __init__(self, num_chunks, chunk_bits, memories, g_terms):
        self.c, self.l, self.memories = num_chunks, chunk_bits, list(memories)
        self.g_terms = [(co % R_MOD, list(f)) for co, f in g_terms]

    @classmethod
    def range(cls, num_chunks=2, chunk_bits=16):
        return cls(num_chunks, chunk_bits, [(j, SUBTABLE_IDENTITY) for j in range(num_chunks)],
                   [(1 << (chunk_bits * j), [j]) for j in range(num_chunks)])

    @classmethod
    def bitwise(cls, kind, num_chunks=4, chunk_bits=16):
        return cls(num_chunks, chunk_bits, [(j, kind) for j in range(num_chunks)],
                   [(1 << (chunk_bits // 2 * j), [j]) for j in range(num_chunks)])

    @classmethod
    def equal(cls, num_chunks=4, chunk_bits=16):
        """x == y for two (c*l/2)-bit operands, chunk j = x_j || y_j (chunk 0 least significant): g = prod_j EQ_j.  The
        term has c factors: c <= LH_SC_MAX_FACTORS."""
        if not 1 <= num_chunks <= _ffi.LH_SC_MAX_FACTORS:
            raise ArgumentError("equal: 1 to %d chunks (one factor of g each)" % _ffi.LH_SC_MAX_FACTORS)
        return cls(num_chunks, chunk_bits, [(j, SUBTABLE_EQ) for j in range(num_chunks)], [(1, list(range(num_chunks)))])

    @classmethod
    def less_than(cls, num_chunks=4, chunk_bits=16):
        """x < y (unsigned) for two (c*l/2)-bit operands, chunk j = x_j || y_j (chunk 0 least significant): memories
        LTU_0..LTU_{c-1}, then EQ_1..EQ_{c-1} (alpha = 2c - 1); g = sum_j LTU_j prod_{k > j} EQ_k - the highest chunk that
        differs decides.  The longest term has c factors: c <= LH_SC_MAX_FACTORS (c = 4, l = 16: 32-bit operands)."""
        if not 1 <= num_chunks <= _ffi.LH_SC_MAX_FACTORS:
            raise ArgumentError("less_than: 1 to %d chunks (the longest term of g has one factor each)" % _ffi.LH_SC_MAX_FACTORS)
        c = num_chunks
        memories = [(j, SUBTABLE_LTU) for j in range(c)] + [(j, SUBTABLE_EQ) for j in range(1, c)]
        return cls(c, chunk_bits, memories, [(1, [j] + [c + k - 1 for k in range(j + 1, c)]) for j in range(c)])

    @classmethod
    def less_than_signed(cls, num_chunks=4, chunk_bits=16):
        """sx < sy for two two's-complement (c*l/2)-bit operands: less_than's shape with the top chunk's LTU replaced by a
        registered subtable, (sx < sy) on the signed l/2-bit halves of that chunk (below the top chunk the comparison is the
        unsigned one).  That subtable has T[0] = 0; it is registered once per chunk_bits and kept for the process."""
        if not 1 <= num_chunks <= _ffi.LH_SC_MAX_FACTORS:
            raise ArgumentError("less_than_signed: 1 to %d chunks (the longest term of g has one factor each)" % _ffi.LH_SC_MAX_FACTORS)
        if chunk_bits % 2 or not 2 <= chunk_bits <= _ffi.LH_SUBTABLE_CUSTOM_MAX_BITS:
            raise ArgumentError("less_than_signed: an even chunk_bits in [2, %d]" % _ffi.LH_SUBTABLE_CUSTOM_MAX_BITS)
        if chunk_bits not in _LTS_SUBTABLES:
            h = chunk_bits // 2
            signed = lambda v: v - (1 << h) if v >> (h - 1) else v
            _LTS_SUBTABLES[chunk_bits] = Subtable.register(
                [int(signed(m >> h) < signed(m & ((1 << h) - 1))) for m in range(1 << chunk_bits)])
        c = num_chunks
        memories = [(j, SUBTABLE_LTU) for j in range(c - 1)] + [(c - 1, _LTS_SUBTABLES[chunk_bits])] \
            + [(j, SUBTABLE_EQ) for j in range(1, c)]
        return cls(c, chunk_bits, memories, [(1, [j] + [c + k - 1 for k in range(j + 1, c)]) for j in range(c)])

    def check(self):
        """what to_c cannot express, or the library refuses anyway: ArgumentError before anything is marshalled"""
        if len(self.memories) > _ffi.LH_LASSO_MAX_MEMORIES or self.c > _ffi.LH_LASSO_MAX_CHUNKS \
                or len(self.g_terms) > _ffi.LH_LASSO_MAX_TERMS:
            raise ArgumentError("table too large")
        for _, kind in self.memories:
            kind = int(kind)
            if 0 <= kind <= SUBTABLE_LTU:
                continue
            if kind < _ffi.LH_SUBTABLE_CUSTOM_BASE:
                raise ArgumentError("lasso: unknown subtable")
            cb = C.c_uint32()  # a registered kind, and of this table's chunk size
            if _ffi.load().lh_subtable_info(kind, C.byref(cb), None, None) != _ffi.LH_OK:
                raise ArgumentError("lasso: subtable kind %d is not registered" % kind)
            if cb.value != self.l:
                raise ArgumentError("lasso: chunk_bits %d differs from the registered subtable's %d" % (self.l, cb.value))
        if any(not 1 <= len(facs) <= _ffi.LH_SC_MAX_FACTORS for _, facs in self.g_terms):
            raise ArgumentError("lasso: bad g term")

    def to_c(self):
        self.check()
        t = lh_lasso_table()
        t.num_chunks, t.chunk_bits, t.num_memories = self.c, self.l, len(self.memories)
        for i, (j, kind) in enumerate(self.memories):
            t.memory_chunk[i], t.memory_subtable[i] = j, int(kind)
        t.num_terms = len(self.g_terms)
        for m, (co, facs) in enumerate(self.g_terms):
            C.memmove(C.byref(t.g_coeff[m]), fr_to_bytes(co), 32)
            t.g_num_factors[m] = len(facs)
            for k, f in enumerate(facs):
                t.g_factor[m][k] = f
        return t


def lasso_prove(pp, table, num_vars, dims, transcript):
    """dims: c device buffers of u32[2^num_vars] chunk indices. Appends the proof to `transcript`."""
    if len(dims) != table.c:
        raise ArgumentError("expected %d dim columns" % table.c)
    t = table.to_c()
    _check(getattr(pp.ctx.lib, "lh_lasso_prove" + pp.suffix)(pp.ctx.h, *pp.head(), C.byref(t), num_vars, _ptr_array(dims),
                                                             transcript.p, *_tail(pp, transcript)))


def _table_list(tables):
    """K tables as the `const lh_lasso_table* const*` of the batch entries -> (pointer array, keepalive)"""
    if not 1 <= len(tables) <= _ffi.LH_LASSO_BATCH_MAX_TABLES:
        raise ArgumentError("lasso batch: 1 to %d tables" % _ffi.LH_LASSO_BATCH_MAX_TABLES)
    cs = [t.to_c() for t in tables]
    arr = (C.POINTER(lh_lasso_table) * len(cs))(*[C.pointer(c) for c in cs])
    return arr, cs


def lasso_prove_batch(pp, tables, num_vars, dims, transcript):
    """Lookups into several tables in ONE proof over multilinear KZG (include/lasso_hip.h lh_lasso_prove_batch):
    tables: K LassoTable; dims[t]: the c_t device buffers of u32[2^num_vars] chunk indices of table t.  Two tables of equal
    chunk_bits handed the same buffer for a chunk column share that column's counters and commitments."""
    if len(dims) != len(tables):
        raise ArgumentError("expected one list of dim columns per table")
    for t, (table, cols) in enumerate(zip(tables, dims)):
        if len(cols) != table.c:
            raise ArgumentError("table %d: expected %d dim columns" % (t, table.c))
    arr, keep = _table_list(tables)
    cols = [_ptr_array(d) for d in dims]
    col_arr = (C.POINTER(C.c_void_p) * len(cols))(*[C.cast(c, C.POINTER(C.c_void_p)) for c in cols])
    _check(pp.ctx.lib.lh_lasso_prove_batch(pp.ctx.h, pp.h, arr, len(tables), num_vars, col_arr, transcript.p))
    del keep


# ------------------------------------------------------------------ LogUp-GKR (include/lasso_hip.h lh_logup_gkr_prove)
class U32Column:
    """An input column of a LogUp-GKR lookup held as uint32_t[2^num_vars] in a DeviceBuffer: the same polynomial as the
    values widened to Fr - and the same proof bytes - committed, compressed, evaluated and opened as a 32-bit column."""

    def __init__(self, buf, num_vars):
        self.buf, self.num_vars = buf, num_vars

    @property
    def ptr(self):
        return self.buf.ptr


class LogupLookup:
    """One lookup of a LogUp-GKR proof: `inputs`, w device columns (MultilinearPolynomial / DeviceBuffer of 2^num_vars Fr, or
    U32Column, in any mix; None for a verifier), looked up by value in `table`, w lists of 2^table_vars ints - a row is a
    tuple of w elements."""

    def __init__(self, inputs, table):
        self.inputs = None if inputs is None else list(inputs)
        self.table = [list(col) for col in table]

    @property
    def width(self):
        return len(self.table)

    @property
    def table_vars(self):
        return len(self.table[0]).bit_length() - 1 if self.table and self.table[0] else 0

    def check(self, prover):
        """ArgumentError before anything is marshalled or the device is touched"""
        if not 1 <= self.width <= _ffi.LH_LOGUP_MAX_WIDTH:
            raise ArgumentError("logup: width out of range (1 to %d)" % _ffi.LH_LOGUP_MAX_WIDTH)
        rows = len(self.table[0])
        if rows < 2 or rows & (rows - 1) or any(len(col) != rows for col in self.table):
            raise ArgumentError("logup: table columns of one power-of-two length >= 2")
        if self.table_vars > _ffi.LH_LOGUP_MAX_TABLE_VARS:
            raise ArgumentError("logup: table_vars out of range (1 to %d)" % _ffi.LH_LOGUP_MAX_TABLE_VARS)
        if prover and (self.inputs is None or len(self.inputs) != self.width):
            raise ArgumentError("logup: expected %d input columns" % self.width)


def _logup_list(lookups, num_vars, prover, columns=False):
    """-> (lh_logup_lookup array, table_vars, keepalive); columns: an lh_logup_columns array, U32Column inputs allowed"""
    if not 1 <= len(lookups) <= _ffi.LH_LOGUP_MAX_LOOKUPS:
        raise ArgumentError("logup: 1 to %d lookups" % _ffi.LH_LOGUP_MAX_LOOKUPS)
    for lk in lookups:
        lk.check(prover)
    table_vars = lookups[0].table_vars
    if any(lk.table_vars != table_vars for lk in lookups):
        raise ArgumentError("logup: every table has 2^table_vars rows")
    if not 1 <= num_vars < 31:
        raise ArgumentError("logup: num_vars out of range (1 to 30)")
    if sum(lk.width for lk in lookups) > 63:
        raise ArgumentError("logup: more than 63 input columns in all (one identity mask)")
    arr, keep = ((_ffi.lh_logup_columns if columns else _ffi.lh_logup_lookup) * len(lookups))(), []
    for k, lk in enumerate(lookups):
        cols = [_fr_array(col) for col in lk.table]
        tab = (C.POINTER(lh_fr) * lk.width)(*[C.cast(col, C.POINTER(lh_fr)) for col in cols])
        arr[k].width, arr[k].table = lk.width, tab
        keep += [cols, tab]
        if prover:
            if any(getattr(p, "num_vars", num_vars) != num_vars for p in lk.inputs):
                raise ArgumentError("logup: input columns of 2^num_vars entries")
            for j, p in enumerate(lk.inputs):
                if isinstance(p, U32Column) and getattr(p.buf, "nbytes", 4 << num_vars) < 4 << num_vars:
                    raise ArgumentError("logup: lookup %d, column %d: a u32 column of 2^num_vars entries needs %d bytes"
                                        % (k, j, 4 << num_vars))
            if columns:
                kinds = (C.c_uint8 * lk.width)(*[_ffi.LH_LOGUP_COL_U32 if isinstance(p, U32Column) else _ffi.LH_LOGUP_COL_FR
                                                 for p in lk.inputs])
                arr[k].kinds = kinds
                keep.append(kinds)
            ins = _ptr_array(lk.inputs)
            arr[k].d_inputs = C.cast(ins, C.POINTER(C.c_void_p))
            keep.append(ins)
    return arr, table_vars, keep


def logup_gkr_prove(pp, lookups, transcript, num_vars=None):
    """LogUp-GKR over multilinear KZG (tests/logup_gkr_ref.py): every input row of every lookup is a row of its table.
    num_vars: of the input columns (default: the first column's, a MultilinearPolynomial or U32Column).  Inputs that are
    U32Column go through lh_logup_gkr_prove_columns; the bytes do not depend on the kinds.  Appends the proof."""
    if num_vars is None:
        if not lookups or not lookups[0].inputs or not hasattr(lookups[0].inputs[0], "num_vars"):
            raise ArgumentError("logup: num_vars is needed with raw device buffers")
        num_vars = lookups[0].inputs[0].num_vars
    columns = any(isinstance(p, U32Column) for lk in lookups for p in (lk.inputs or ()))
    arr, table_vars, keep = _logup_list(lookups, num_vars, True, columns)
    prove = pp.ctx.lib.lh_logup_gkr_prove_columns if columns else pp.ctx.lib.lh_logup_gkr_prove
    _check(prove(pp.ctx.h, pp.h, arr, len(lookups), num_vars, table_vars, transcript.p))
    del keep


def logup_gkr_verify(vp, lookups, num_vars, transcript):
    """Verifier of logup_gkr_prove (host only; the lookups' inputs are ignored).  A Keccak256Transcript must be fully
    consumed."""
    arr, table_vars, keep = _logup_list(lookups, num_vars, False)
    _check(vp.lib.lh_logup_gkr_verify(vp.h, arr, len(lookups), num_vars, table_vars, transcript.p))
    del keep
    if isinstance(transcript, Keccak256Transcript) and transcript.remaining():
        raise InvalidSnark("trailing bytes in proof")


# ------------------------------------------------------------------ read-write memory checking (lh_memcheck_prove)
def _memcheck_statement(num_vars, mem_vars, init):
    """ArgumentError before anything is marshalled or the device is touched -> the image as a uint32 array, or None"""
    if not (isinstance(num_vars, int) and 1 <= num_vars < 31):
        raise ArgumentError("memcheck: num_vars out of range (1 to 30)")
    top = _ffi.LH_MEMCHECK_MAX_INIT_VARS if init is not None else 30
    if not (isinstance(mem_vars, int) and 1 <= mem_vars <= top):
        raise ArgumentError("memcheck: mem_vars out of range (1 to %d)" % top)
    if init is None:
        return None
    if len(init) != 1 << mem_vars:
        raise ArgumentError("memcheck: an initial image of 2^mem_vars words")
    if isinstance(init, C.Array) and init._type_ is C.c_uint32:  # (marshalled by the caller, once for many calls)
        return init
    if any(not 0 <= v < 1 << 32 for v in init):
        raise ArgumentError("memcheck: the words of the image are 32-bit")
    return (C.c_uint32 * len(init))(*init)


def _memcheck_trace(addr, rv, wv, num_vars):
    """-> (lh_memcheck_trace, num_vars); the columns are u32 DeviceBuffers or U32Columns of 2^num_vars entries"""
    cols = (addr, rv, wv)
    if any(c is None for c in cols):
        raise ArgumentError("memcheck: the trace is three columns, addr, rv and wv")
    if num_vars is None:
        if not hasattr(addr, "num_vars"):
            raise ArgumentError("memcheck: num_vars is needed with raw device buffers")
        num_vars = addr.num_vars
    if any(getattr(c, "num_vars", num_vars) != num_vars for c in cols):
        raise ArgumentError("memcheck: trace columns of 2^num_vars entries")
    if isinstance(num_vars, int) and 1 <= num_vars < 31:
        for c in cols:
            if getattr(getattr(c, "buf", c), "nbytes", 4 << num_vars) < 4 << num_vars:
                raise ArgumentError("memcheck: a trace column of 2^num_vars entries needs %d bytes" % (4 << num_vars))
    trace = _ffi.lh_memcheck_trace()
    trace.d_addr, trace.d_rv, trace.d_wv = [C.cast(C.c_void_p(c.ptr if hasattr(c, "ptr") else c), C.POINTER(C.c_uint32))
                                            for c in cols]
    return trace, num_vars


def memcheck_prove(pp, addr, rv, wv, mem_vars, transcript, init=None, num_vars=None):
    """Read-write memory checking over multilinear KZG (tests/memcheck_ref.py): the trace addr / rv / wv - u32 DeviceBuffers
    or U32Columns of 2^num_vars entries - is consistent over a memory of 2^mem_vars 32-bit cells that starts as `init`
    (2^mem_vars ints, or a ctypes c_uint32 array marshalled once by the caller; None: all zero): every rv is the wv of the latest earlier operation on its cell, or the image's
    word.  An inconsistent trace or an address >= 2^mem_vars: InvalidSnark "Invalid memory trace".  Appends the proof."""
    trace, num_vars = _memcheck_trace(addr, rv, wv, num_vars)
    image = _memcheck_statement(num_vars, mem_vars, init)
    _check(pp.ctx.lib.lh_memcheck_prove(pp.ctx.h, pp.h, C.byref(trace), num_vars, mem_vars, image, transcript.p))


def memcheck_verify(vp, num_vars, mem_vars, transcript, init=None):
    """Verifier of memcheck_prove (host only).  A Keccak256Transcript must be fully consumed."""
    image = _memcheck_statement(num_vars, mem_vars, init)
    _check(vp.lib.lh_memcheck_verify(vp.h, num_vars, mem_vars, image, transcript.p))
    if isinstance(transcript, Keccak256Transcript) and transcript.remaining():
        raise InvalidSnark("trailing bytes in proof")


def memcheck_witness(ctx, addr, rv, wv, mem_vars, init=None, num_vars=None):
    """(development) the witness kernels of memcheck_prove alone (lh_debug_memcheck_witness) -> (rt, fv, ft, m, bad): the
    previous-write times, the final values and times of the cells, the multiplicities of i - rt[i] as lists of ints, and
    whether the trace is invalid (the lists are then unspecified)."""
    import array
    trace, num_vars = _memcheck_trace(addr, rv, wv, num_vars)
    image = _memcheck_statement(num_vars, mem_vars, init)
    sizes = [4 << num_vars, 4 << mem_vars, 4 << mem_vars, 4 << num_vars]
    bufs = [ctx.alloc(s) for s in sizes]
    bad = C.c_int(0)
    _check(ctx.lib.lh_debug_memcheck_witness(ctx.h, C.byref(trace), num_vars, mem_vars, image, *[b.ptr for b in bufs],
                                             C.byref(bad)))
    out = [array.array("I", b.read()).tolist() for b in bufs]
    for b in bufs:
        b.free()
    return out[0], out[1], out[2], out[3], bool(bad.value)


def _memcheck_shape(num_vars, mem_vars):
    """the limits without a public image (lh_memcheck_replay, the segment proofs): ArgumentError before the device is touched"""
    if not (isinstance(num_vars, int) and 1 <= num_vars < 31):
        raise ArgumentError("memcheck: num_vars out of range (1 to 30)")
    if not (isinstance(mem_vars, int) and 1 <= mem_vars < 31):
        raise ArgumentError("memcheck: mem_vars out of range (1 to 30)")


def _u32_ptr(col, words, what):
    """a device column of at least `words` uint32 (DeviceBuffer or U32Column; a raw pointer is taken as it is) -> c_void_p"""
    buf = getattr(col, "buf", col)
    if getattr(buf, "nbytes", 4 * words) < 4 * words:
        raise ArgumentError("memcheck: %s needs %d bytes" % (what, 4 * words))
    return C.c_void_p(col.ptr if hasattr(col, "ptr") else col)


def memcheck_replay(ctx, addr, store, val, mem_vars, image=None, num_vars=None):
    """The trace from the operations, on the device (lh_memcheck_replay): addr / store / val are u32 DeviceBuffers or
    U32Columns of 2^num_vars entries - operation i stores val[i] when store[i] != 0, else it loads -, image a u32 device
    column of 2^mem_vars words or None (all zero).  -> (rv, wv, final) as U32Columns on the device (final: mem_vars
    variables): rv[i] is the word of the latest earlier store to addr[i], or the image's; wv[i] = val[i] for a store, rv[i] for
    a load; final[a] the cell's word after the trace.  (addr, rv, wv) is what memcheck_prove and memcheck_prove_segment take.
    An address >= 2^mem_vars: InvalidSnark "Invalid memory trace"."""
    if any(c is None for c in (addr, store, val)):
        raise ArgumentError("memcheck: the operations are three columns, addr, store and val")
    if num_vars is None:
        if not hasattr(addr, "num_vars"):
            raise ArgumentError("memcheck: num_vars is needed with raw device buffers")
        num_vars = addr.num_vars
    _memcheck_shape(num_vars, mem_vars)
    if any(getattr(c, "num_vars", num_vars) != num_vars for c in (addr, store, val)):
        raise ArgumentError("memcheck: operation columns of 2^num_vars entries")
    ops = _ffi.lh_memcheck_ops()
    ops.d_addr, ops.d_store, ops.d_val = [C.cast(_u32_ptr(c, 1 << num_vars, "an operation column"), C.POINTER(C.c_uint32))
                                          for c in (addr, store, val)]
    d_image = _u32_ptr(image, 1 << mem_vars, "the image") if image is not None else None
    rv, wv, final = ctx.alloc(4 << num_vars), ctx.alloc(4 << num_vars), ctx.alloc(4 << mem_vars)
    try:
        _check(ctx.lib.lh_memcheck_replay(ctx.h, C.byref(ops), num_vars, mem_vars, d_image, rv.ptr, wv.ptr, final.ptr))
    except Exception:
        for b in (rv, wv, final):
            b.free()
        raise
    return U32Column(rv, num_vars), U32Column(wv, num_vars), U32Column(final, mem_vars)


def memcheck_prove_segment(pp, addr, rv, wv, mem_vars, image, transcript, num_vars=None, final=None):
    """One segment of a memory-checking chain over multilinear KZG (tests/memcheck_segment_ref.py): memcheck_prove with the
    image as a COMMITTED column - `image` is a u32 device column of 2^mem_vars words, never None - so that the next segment
    can start from this one's final values.  final: a u32 device column of 2^mem_vars words that receives them (None: one is
    allocated).  Appends the proof; -> the final values as a U32Column on the device."""
    trace, num_vars = _memcheck_trace(addr, rv, wv, num_vars)
    _memcheck_shape(num_vars, mem_vars)
    if image is None:
        raise ArgumentError("memcheck: a segment needs its image, a device column of 2^mem_vars words")
    d_image = _u32_ptr(image, 1 << mem_vars, "the image")
    out = final if final is not None else U32Column(pp.ctx.alloc(4 << mem_vars), mem_vars)
    d_final = _u32_ptr(out, 1 << mem_vars, "the final values")
    _check(pp.ctx.lib.lh_memcheck_prove_segment(pp.ctx.h, pp.h, C.byref(trace), num_vars, mem_vars, d_image, d_final, transcript.p))
    return out


def memcheck_verify_segment(vp, num_vars, mem_vars, transcript):
    """Verifier of memcheck_prove_segment (host only) -> (image commitment, final commitment) as read from the proof: affine
    (x, y), None for the identity (an all-zero column).  A Keccak256Transcript must be fully consumed."""
    _memcheck_shape(num_vars, mem_vars)
    iv, fv = lh_g1(), lh_g1()
    _check(vp.lib.lh_memcheck_verify_segment(vp.h, num_vars, mem_vars, transcript.p, C.byref(iv), C.byref(fv)))
    if isinstance(transcript, Keccak256Transcript) and transcript.remaining():
        raise InvalidSnark("trailing bytes in proof")
    return g1_from_bytes(bytes(iv)), g1_from_bytes(bytes(fv))


def memcheck_verify_chain(vp, mem_vars, segments):
    """A chain of segment proofs over one memory: segments = [(num_vars, proof bytes), ..] in order.  Verifies every segment
    and requires segment k + 1's image commitment to equal segment k's final commitment -> (first image commitment, last
    final commitment).  A column's commitment depends on the number of variables it is committed over, so segments that
    differ in max(num_vars, mem_vars) can never link: ArgumentError."""
    segments = list(segments)
    if not segments:
        raise ArgumentError("memcheck chain: no segment")
    for num_vars, _ in segments:
        _memcheck_shape(num_vars, mem_vars)
    if len({max(num_vars, mem_vars) for num_vars, _ in segments}) != 1:
        raise ArgumentError("memcheck chain: the segments differ in max(num_vars, mem_vars), their commitments cannot link")
    first = last = None
    for k, (num_vars, proof) in enumerate(segments):
        iv, fv = memcheck_verify_segment(vp, num_vars, mem_vars, Keccak256Transcript.from_proof(proof))
        if k == 0:
            first = iv
        elif iv != last:
            raise InvalidSnark("memcheck chain: segment %d does not start where segment %d ends" % (k, k - 1))
        last = fv
    return first, last


# ------------------------------------------------------------------ Spark: sparse polynomial commitment (lh_spark_commit)
def _spark_shape(num_vars, dim_vars, num_dims):
    """ArgumentError before anything is marshalled or the device is touched"""
    if not (isinstance(num_dims, int) and 1 <= num_dims <= _ffi.LH_SPARK_MAX_DIMS):
        raise ArgumentError("spark: num_dims out of range (1 to %d)" % _ffi.LH_SPARK_MAX_DIMS)
    if not (isinstance(dim_vars, int) and 1 <= dim_vars <= _ffi.LH_SPARK_MAX_DIM_VARS):
        raise ArgumentError("spark: dim_vars out of range (1 to %d)" % _ffi.LH_SPARK_MAX_DIM_VARS)
    if not (isinstance(num_vars, int) and 1 <= num_vars < 31):
        raise ArgumentError("spark: num_vars out of range (1 to 30)")


class SparkPoly:
    """A committed sparse multilinear polynomial (`lh_spark_poly`): owns device copies of its entries, the access counters
    and the commitment.  Open it any number of times with spark_open; free() (or `with`) gives the device memory back -
    it also goes with the ctx.  `commitment`: the bytes spark_verify takes."""

    def __init__(self, ctx, h, num_vars, dim_vars, num_dims):
        self.ctx, self.h, self.num_vars, self.dim_vars, self.num_dims = ctx, h, num_vars, dim_vars, num_dims
        n = C.c_size_t(0)
        _check(ctx.lib.lh_spark_commitment(h, None, C.byref(n)))
        out = (C.c_uint8 * n.value)()
        _check(ctx.lib.lh_spark_commitment(h, out, C.byref(n)))
        self.commitment = bytes(out[:n.value])

    def free(self):
        if self.h and self.ctx.h:  # (a ctx that is gone has taken its polynomials with it)
            self.ctx.lib.lh_spark_free(self.ctx.h, self.h)
        self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def spark_commit(ctx, srs, dims, val, dim_vars, num_vars=None):
    """Commit the sparse polynomial sum_k val[k] prod_j eq(r_j, dims[j][k]) in len(dims) * dim_vars variables over
    multilinear KZG (tests/spark_ref.py): `dims` are 1 to 3 u32 columns (U32Column / DeviceBuffer, 2^num_vars indices below
    2^dim_vars), `val` a MultilinearPolynomial or DeviceBuffer of 2^num_vars Fr.  An index out of range: ArgumentError."""
    dims = list(dims) if dims is not None else []
    if val is None or any(d is None for d in dims):
        raise ArgumentError("spark: null argument: dims or val")
    if num_vars is None:
        if not hasattr(val, "num_vars"):
            raise ArgumentError("spark: num_vars is needed with raw device buffers")
        num_vars = val.num_vars
    _spark_shape(num_vars, dim_vars, len(dims))
    if any(getattr(p, "num_vars", num_vars) != num_vars for p in dims + [val]):
        raise ArgumentError("spark: columns of 2^num_vars entries")
    for p, width in [(d, 4) for d in dims] + [(val, 32)]:
        if getattr(getattr(p, "buf", p), "nbytes", width << num_vars) < width << num_vars:
            raise ArgumentError("spark: a column of 2^num_vars entries needs %d bytes" % (width << num_vars))
    cols = _ptr_array(dims)
    h = C.c_void_p()
    _check(ctx.lib.lh_spark_commit(ctx.h, srs.h, num_vars, dim_vars, len(dims), C.cast(cols, C.POINTER(C.POINTER(C.c_uint32))),
                                   C.cast(C.c_void_p(val.ptr if hasattr(val, "ptr") else val), C.POINTER(lh_fr)), C.byref(h)))
    return SparkPoly(ctx, h, num_vars, dim_vars, len(dims))


def spark_open(ctx, srs, poly, point, transcript=None):
    """Prove the evaluation of a SparkPoly at `point` (num_dims * dim_vars ints) -> (value, proof bytes); with a transcript
    given the proof is appended to it and (value, None) returned."""
    if not isinstance(poly, SparkPoly) or not poly.h:
        raise ArgumentError("spark: the polynomial has been freed")
    if len(point) != poly.num_dims * poly.dim_vars:
        raise ArgumentError("spark: a point of num_dims * dim_vars coordinates")
    t = transcript if transcript is not None else Keccak256Transcript()
    out = (lh_fr * 1)()
    _check(ctx.lib.lh_spark_open(ctx.h, srs.h, poly.h, _fr_array(point), out, t.p))
    return _fr_list(out, 1)[0], (t.into_proof() if transcript is None else None)


def spark_verify(vp, num_vars, dim_vars, num_dims, commitment, point, value, proof):
    """Verifier of spark_open (host only): `commitment` the bytes of SparkPoly.commitment, `proof` bytes or a transcript.
    A Keccak256Transcript must be fully consumed."""
    _spark_shape(num_vars, dim_vars, num_dims)
    if commitment is None or point is None or value is None or proof is None:
        raise ArgumentError("spark: null argument")
    if len(point) != num_dims * dim_vars:
        raise ArgumentError("spark: a point of num_dims * dim_vars coordinates")
    t = Keccak256Transcript.from_proof(bytes(proof)) if isinstance(proof, (bytes, bytearray)) else proof
    blob = (C.c_uint8 * max(len(commitment), 1)).from_buffer_copy(bytes(commitment) or b"\0")
    _check(vp.lib.lh_spark_verify(vp.h, num_vars, dim_vars, num_dims, blob, len(commitment), _fr_array(point),
                                  _fr_array([value]), t.p))
    if isinstance(t, Keccak256Transcript) and t.remaining():
        raise InvalidSnark("trailing bytes in proof")


def spark_e(ctx, dims, val, dim_vars, point, num_vars=None):
    """(development) the memory kernel of spark_open alone (lh_debug_spark_e) -> (E, value): the num_dims memories
    E[j][k] = eq(r_j, dims[j][k]) as lists of ints and sum_k val[k] prod_j E[j][k]."""
    dims = list(dims)
    num_vars = val.num_vars if num_vars is None else num_vars
    _spark_shape(num_vars, dim_vars, len(dims))
    if len(point) != len(dims) * dim_vars:
        raise ArgumentError("spark: a point of num_dims * dim_vars coordinates")
    bufs = [ctx.alloc(32 << num_vars) for _ in dims]
    out = (lh_fr * 1)()
    _check(ctx.lib.lh_debug_spark_e(ctx.h, num_vars, dim_vars, len(dims), C.cast(_ptr_array(dims), C.POINTER(C.POINTER(C.c_uint32))),
                                    C.cast(C.c_void_p(val.ptr if hasattr(val, "ptr") else val), C.POINTER(lh_fr)), _fr_array(point),
                                    C.cast(_ptr_array(bufs), C.POINTER(C.POINTER(lh_fr))), out))
    E = [frs_from_bytes(b.read()) for b in bufs]
    for b in bufs:
        b.free()
    return E, _fr_list(out, 1)[0]


# ------------------------------------------------------------------ Spartan: R1CS over the Spark-committed matrices (lh_r1cs_commit)
def _spartan_shape(num_vars, dim_vars, num_public):
    """ArgumentError before anything is marshalled or the device is touched"""
    lo, hi = _ffi.LH_SPARTAN_MIN_DIM_VARS, _ffi.LH_SPARTAN_MAX_DIM_VARS
    if not (isinstance(dim_vars, int) and lo <= dim_vars <= hi):
        raise ArgumentError("spartan: dim_vars out of range (%d to %d)" % (lo, hi))
    if not (isinstance(num_vars, int) and 1 <= num_vars < 31):
        raise ArgumentError("spartan: num_vars out of range (1 to 30)")
    if not (isinstance(num_public, int) and 1 <= num_public <= 1 << (dim_vars - 1)):
        raise ArgumentError("spartan: num_public out of range (1 to 2^(dim_vars - 1))")


def _raw_ptr(p):
    return p.ptr if hasattr(p, "ptr") else p


class R1csKey:
    """The key of an R1CS instance (`lh_r1cs_key`): the Spark commitments of A, B, C and their entries sorted by row and by
    column, on the device.  Prove any number of assignments with spartan_prove; free() (or `with`) gives the device memory
    back - it also goes with the ctx.  `commitment`: the bytes spartan_verify takes."""

    def __init__(self, ctx, h, num_vars, dim_vars):
        self.ctx, self.h, self.num_vars, self.dim_vars = ctx, h, num_vars, dim_vars
        n = C.c_size_t(0)
        _check(ctx.lib.lh_r1cs_commitment(h, None, C.byref(n)))
        out = (C.c_uint8 * n.value)()
        _check(ctx.lib.lh_r1cs_commitment(h, out, C.byref(n)))
        self.commitment = bytes(out[:n.value])

    def free(self):
        if self.h and self.ctx.h:  # (a ctx that is gone has taken its keys with it)
            self.ctx.lib.lh_r1cs_free(self.ctx.h, self.h)
        self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def r1cs_commit(ctx, srs, matrices, dim_vars, num_vars=None):
    """The key of the R1CS instance A, B, C over multilinear KZG (tests/spartan_ref.py): `matrices` are three
    (row, col, val) - row, col u32 columns (U32Column / DeviceBuffer, 2^num_vars indices below 2^dim_vars), val a
    MultilinearPolynomial or DeviceBuffer of 2^num_vars Fr.  An index out of range: ArgumentError."""
    matrices = [tuple(m) if m is not None else () for m in matrices] if matrices is not None else []
    if len(matrices) != 3 or any(len(m) != 3 or any(col is None for col in m) for m in matrices):
        raise ArgumentError("spartan: three matrices of (row, col, val)")
    if num_vars is None:
        if not hasattr(matrices[0][2], "num_vars"):
            raise ArgumentError("spartan: num_vars is needed with raw device buffers")
        num_vars = matrices[0][2].num_vars
    _spartan_shape(num_vars, dim_vars, 1)
    for m in matrices:
        if any(getattr(col, "num_vars", num_vars) != num_vars for col in m):
            raise ArgumentError("spartan: columns of 2^num_vars entries, the same for the three matrices")
        for col, width in zip(m, (4, 4, 32)):
            if getattr(getattr(col, "buf", col), "nbytes", width << num_vars) < width << num_vars:
                raise ArgumentError("spartan: a column of 2^num_vars entries needs %d bytes" % (width << num_vars))
    ms = (_ffi.lh_r1cs_matrix * 3)()
    for i, (row, col, val) in enumerate(matrices):
        ms[i].d_row = C.cast(C.c_void_p(_raw_ptr(row)), C.POINTER(C.c_uint32))
        ms[i].d_col = C.cast(C.c_void_p(_raw_ptr(col)), C.POINTER(C.c_uint32))
        ms[i].d_val = C.cast(C.c_void_p(_raw_ptr(val)), C.POINTER(lh_fr))
    h = C.c_void_p()
    _check(ctx.lib.lh_r1cs_commit(ctx.h, srs.h, num_vars, dim_vars, ms, C.byref(h)))
    return R1csKey(ctx, h, num_vars, dim_vars)


def spartan_prove(ctx, srs, key, w, x, transcript=None):
    """Prove that z = (w, x, 0) satisfies the instance of `key`: `w` a MultilinearPolynomial or DeviceBuffer of
    2^(dim_vars - 1) Fr, `x` the public inputs (ints, x[0] the constant 1 if the instance uses one) -> the proof bytes; with a
    transcript given the proof is appended to it and None returned.  A witness that does not satisfy: ArgumentError."""
    if not isinstance(key, R1csKey) or not key.h:
        raise ArgumentError("spartan: the key has been freed")
    if w is None or x is None:
        raise ArgumentError("spartan: null argument: w or x")
    x = list(x)
    _spartan_shape(key.num_vars, key.dim_vars, len(x))
    if getattr(w, "num_vars", key.dim_vars - 1) != key.dim_vars - 1:
        raise ArgumentError("spartan: a witness of 2^(dim_vars - 1) entries")
    if getattr(getattr(w, "buf", w), "nbytes", 32 << (key.dim_vars - 1)) < 32 << (key.dim_vars - 1):
        raise ArgumentError("spartan: a witness of 2^(dim_vars - 1) entries needs %d bytes" % (32 << (key.dim_vars - 1)))
    t = transcript if transcript is not None else Keccak256Transcript()
    _check(ctx.lib.lh_spartan_prove(ctx.h, srs.h, key.h, C.cast(C.c_void_p(_raw_ptr(w)), C.POINTER(lh_fr)), _fr_array(x), len(x),
                                    t.p))
    return t.into_proof() if transcript is None else None


def spartan_verify(vp, num_vars, dim_vars, commitment, x, proof):
    """Verifier of spartan_prove (host only): `commitment` the bytes of R1csKey.commitment, `x` the public inputs, `proof`
    bytes or a transcript.  A Keccak256Transcript must be fully consumed."""
    if commitment is None or x is None or proof is None:
        raise ArgumentError("spartan: null argument")
    x = list(x)
    _spartan_shape(num_vars, dim_vars, len(x))
    t = Keccak256Transcript.from_proof(bytes(proof)) if isinstance(proof, (bytes, bytearray)) else proof
    blob = (C.c_uint8 * max(len(commitment), 1)).from_buffer_copy(bytes(commitment) or b"\0")
    _check(vp.lib.lh_spartan_verify(vp.h, num_vars, dim_vars, blob, len(commitment), _fr_array(x), len(x), t.p))
    if isinstance(t, Keccak256Transcript) and t.remaining():
        raise InvalidSnark("spartan: trailing bytes in proof")


def spartan_spmv(ctx, key, direction, x):
    """(development) the keyed field sum of spartan_prove alone (lh_debug_spartan_spmv) -> three lists of 2^dim_vars ints:
    direction 0, M x for M = A, B, C (sums by row); direction 1, M^T x (sums by column).  `x`: 2^dim_vars ints.  The output
    buffers are filled with non-zero bytes first: the kernel owes every cell."""
    if not isinstance(key, R1csKey) or not key.h:
        raise ArgumentError("spartan: the key has been freed")
    if direction not in (0, 1):
        raise ArgumentError("spartan: direction is 0 (by rows) or 1 (by columns)")
    x = list(x)
    if len(x) != 1 << key.dim_vars:
        raise ArgumentError("spartan: a vector of 2^dim_vars entries")
    size = 32 << key.dim_vars
    d_x = ctx.upload(frs_to_bytes(x))
    bufs = [ctx.upload(b"\xa5" * size) for _ in range(3)]
    _check(ctx.lib.lh_debug_spartan_spmv(ctx.h, key.h, direction, C.cast(C.c_void_p(d_x.ptr), C.POINTER(lh_fr)),
                                         C.cast(_ptr_array(bufs), C.POINTER(C.POINTER(lh_fr)))))
    out = [frs_from_bytes(b.read()) for b in bufs]
    for b in bufs + [d_x]:
        b.free()
    return out


# ------------------------------------------------------------------ Nova folding over an R1CS key; relaxed Spartan (tests/nova_ref.py)
def _fr_ptr(p):
    """a device vector (MultilinearPolynomial / DeviceBuffer / raw pointer) or None as lh_fr*"""
    return C.cast(C.c_void_p(_raw_ptr(p)), C.POINTER(lh_fr)) if p is not None else None


def _bytes_arg(b):
    return (C.c_uint8 * max(len(b), 1)).from_buffer_copy(bytes(b) or b"\0")


def _nova_vector(key, p, vars_, what):
    if getattr(p, "num_vars", vars_) != vars_ or getattr(getattr(p, "buf", p), "nbytes", 32 << vars_) < 32 << vars_:
        raise ArgumentError("nova: %s of 2^%d entries (%d bytes)" % (what, vars_, 32 << vars_))


def _nova_key(key, name="nova"):
    if not isinstance(key, R1csKey) or not key.h:
        raise ArgumentError("%s: the key has been freed" % name)


def nova_instance_bytes(num_public):
    """the most bytes an instance blob of num_public public inputs takes (LH_NOVA_INSTANCE_BYTES)"""
    return 160 + 32 * num_public


def _nova_room(instance):
    """the room the fold of `instance` takes: LH_NOVA_INSTANCE_BYTES of its number of public inputs, which follows from its
    mask and its length (a blob that cannot be read is the library's to refuse: any room will do)"""
    points = 2 - bin(instance[31] & 3).count("1") if len(instance) >= 32 else 0
    return nova_instance_bytes(max(len(instance) - 32 - 64 * points, 0) // 32)


def nova_instance(ctx, srs, key, w, x):
    """The fresh relaxed instance of an assignment z = (w, x, 0) that satisfies the instance of `key`, x[0] = 1 -> the
    instance blob (bytes): the commitment of w, C_E the identity, x.  Its witness is (w, None)."""
    _nova_key(key)
    if w is None or x is None:
        raise ArgumentError("nova: null argument: w or x")
    x = list(x)
    _spartan_shape(key.num_vars, key.dim_vars, len(x))
    _nova_vector(key, w, key.dim_vars - 1, "a witness")
    out, n = (C.c_uint8 * nova_instance_bytes(len(x)))(), C.c_size_t(nova_instance_bytes(len(x)))
    _check(ctx.lib.lh_nova_instance(ctx.h, srs.h, key.h, _fr_ptr(w), _fr_array(x), len(x), out, C.byref(n)))
    return bytes(out[:n.value])


def nova_fold(ctx, srs, key, instance1, w1, e1, instance2, w2, e2, w_out, e_out, transcript=None):
    """Fold the relaxed instances (instance1, w1, e1) and (instance2, w2, e2) of `key` - blobs, device vectors of
    2^(dim_vars - 1) and 2^dim_vars Fr, e1 / e2 None for zero - into the caller's w_out and e_out (which may be w1 and e1)
    -> (the folded instance blob, the proof bytes); with a transcript given the proof is appended to it and None returned
    in its place.  An input that fails its own relaxed relation: ArgumentError, nothing written."""
    _nova_key(key)
    if any(v is None for v in (instance1, instance2, w1, w2, w_out, e_out)):
        raise ArgumentError("nova: null argument: an instance, a witness or an output")
    l = key.dim_vars
    for p, vars_, what in ((w1, l - 1, "a witness"), (w2, l - 1, "a witness"), (w_out, l - 1, "a witness"), (e_out, l, "an error vector")) + \
            tuple((e, l, "an error vector") for e in (e1, e2) if e is not None):
        _nova_vector(key, p, vars_, what)
    room = _nova_room(bytes(instance1))
    out, n = (C.c_uint8 * room)(), C.c_size_t(room)
    t = transcript if transcript is not None else Keccak256Transcript()
    _check(ctx.lib.lh_nova_fold(ctx.h, srs.h, key.h, _bytes_arg(instance1), len(instance1), _bytes_arg(instance2), len(instance2),
                                _fr_ptr(w1), _fr_ptr(e1), _fr_ptr(w2), _fr_ptr(e2), _fr_ptr(w_out), _fr_ptr(e_out), out, C.byref(n), t.p))
    return bytes(out[:n.value]), (t.into_proof() if transcript is None else None)


def nova_fold_verify(num_vars, dim_vars, commitment, instance1, instance2, proof, lib=None):
    """Verifier of nova_fold (host only; no param): `commitment` the bytes of R1csKey.commitment, the two instance blobs,
    `proof` bytes or a transcript -> the folded instance blob.  A Keccak256Transcript must be fully consumed."""
    if commitment is None or instance1 is None or instance2 is None or proof is None:
        raise ArgumentError("nova: null argument")
    _spartan_shape(num_vars, dim_vars, 1)
    t = Keccak256Transcript.from_proof(bytes(proof)) if isinstance(proof, (bytes, bytearray)) else proof
    room = _nova_room(bytes(instance1))
    out, n = (C.c_uint8 * room)(), C.c_size_t(room)
    _check((lib or _ffi.load()).lh_nova_fold_verify(num_vars, dim_vars, _bytes_arg(commitment), len(commitment), _bytes_arg(instance1),
                                                    len(instance1), _bytes_arg(instance2), len(instance2), out, C.byref(n), t.p))
    if isinstance(t, Keccak256Transcript) and t.remaining():
        raise InvalidSnark("nova: trailing bytes in proof")
    return bytes(out[:n.value])


def spartan_prove_relaxed(ctx, srs, key, instance, w, e, transcript=None):
    """Prove the relaxed instance `instance` (a blob of nova_instance / nova_fold) of `key` with the witness (w, e), e None
    for an instance whose C_E is the identity -> the proof bytes; with a transcript given the proof is appended to it and
    None returned.  A witness that fails the relaxed relation: ArgumentError."""
    _nova_key(key, "spartan")
    if instance is None or w is None:
        raise ArgumentError("spartan: null argument: the instance or w")
    _nova_vector(key, w, key.dim_vars - 1, "a witness")
    if e is not None:
        _nova_vector(key, e, key.dim_vars, "an error vector")
    t = transcript if transcript is not None else Keccak256Transcript()
    _check(ctx.lib.lh_spartan_prove_relaxed(ctx.h, srs.h, key.h, _bytes_arg(instance), len(instance), _fr_ptr(w), _fr_ptr(e), t.p))
    return t.into_proof() if transcript is None else None


def spartan_verify_relaxed(vp, num_vars, dim_vars, commitment, instance, num_public, proof):
    """Verifier of spartan_prove_relaxed (host only): `commitment` the bytes of R1csKey.commitment, `instance` the blob,
    `proof` bytes or a transcript.  A Keccak256Transcript must be fully consumed."""
    if commitment is None or instance is None or proof is None:
        raise ArgumentError("spartan: null argument")
    _spartan_shape(num_vars, dim_vars, num_public)
    t = Keccak256Transcript.from_proof(bytes(proof)) if isinstance(proof, (bytes, bytearray)) else proof
    _check(vp.lib.lh_spartan_verify_relaxed(vp.h, num_vars, dim_vars, _bytes_arg(commitment), len(commitment), _bytes_arg(instance),
                                            len(instance), num_public, t.p))
    if isinstance(t, Keccak256Transcript) and t.remaining():
        raise InvalidSnark("spartan: trailing bytes in proof")


def nova_spmv2(ctx, key, direction, x1, x2):
    """(development) the keyed field sum with two right-hand sides alone (lh_debug_nova_spmv2) -> (M x1, M x2), each three
    lists of 2^dim_vars ints (direction as spartan_spmv).  x2 `is` x1: one device vector for both.  The output buffers are
    filled with non-zero bytes first: the kernel owes every cell."""
    _nova_key(key)
    if direction not in (0, 1):
        raise ArgumentError("nova: direction is 0 (by rows) or 1 (by columns)")
    if len(x1) != 1 << key.dim_vars or len(x2) != 1 << key.dim_vars:
        raise ArgumentError("nova: vectors of 2^dim_vars entries")
    size = 32 << key.dim_vars
    d_x1 = ctx.upload(frs_to_bytes(list(x1)))
    d_x2 = d_x1 if x2 is x1 else ctx.upload(frs_to_bytes(list(x2)))
    bufs = [ctx.upload(b"\xa5" * size) for _ in range(6)]
    fr_pp = lambda bs: C.cast(_ptr_array(bs), C.POINTER(C.POINTER(lh_fr)))
    try:
        _check(ctx.lib.lh_debug_nova_spmv2(ctx.h, key.h, direction, _fr_ptr(d_x1), _fr_ptr(d_x2), fr_pp(bufs[:3]), fr_pp(bufs[3:])))
        out = [frs_from_bytes(b.read()) for b in bufs]
    finally:
        for b in bufs + [d_x1] + ([d_x2] if d_x2 is not d_x1 else []):
            b.free()
    return out[:3], out[3:]


def nova_cross_term(ctx, dim_vars, mz1, mz2, e1, e2, u1, u2):
    """(development) the cross-term kernel alone (lh_debug_nova_cross_term): mz1, mz2 three lists of 2^dim_vars ints each,
    e1 / e2 lists or None -> (T, [bad1, bad2]).  T's buffer is filled with non-zero bytes first."""
    M = 1 << dim_vars
    ups = [ctx.upload(frs_to_bytes(list(v))) for v in list(mz1) + list(mz2)]
    es = [ctx.upload(frs_to_bytes(list(e))) if e is not None else None for e in (e1, e2)]
    d_t = ctx.upload(b"\xa5" * (32 * M))
    bad = (C.c_size_t * 2)()
    fr_pp = lambda bs: C.cast(_ptr_array(bs), C.POINTER(C.POINTER(lh_fr)))
    try:
        _check(ctx.lib.lh_debug_nova_cross_term(ctx.h, dim_vars, fr_pp(ups[:3]), fr_pp(ups[3:]), _fr_ptr(es[0]), _fr_ptr(es[1]),
                                                _fr_array([u1]), _fr_array([u2]), _fr_ptr(d_t), bad))
        T = frs_from_bytes(d_t.read())
    finally:
        for b in ups + [e for e in es if e is not None] + [d_t]:
            b.free()
    return T, [bad[0], bad[1]]


def nova_fold_vectors(ctx, dim_vars, w1, w2, e1, t, e2, r, in_place=False):
    """(development) the linear-combination kernel alone (lh_debug_nova_fold) -> (w1 + r w2, e1 + r t + r^2 e2) as lists;
    e1 / e2 None for zero.  in_place: the outputs are the buffers of w1 and e1 (e1 given); else fresh buffers filled with
    non-zero bytes."""
    M = 1 << dim_vars
    d = {k: ctx.upload(frs_to_bytes(list(v))) for k, v in (("w1", w1), ("w2", w2), ("e1", e1), ("t", t), ("e2", e2)) if v is not None}
    if in_place:
        d_w, d_e = d["w1"], d["e1"]
    else:
        d_w, d_e = ctx.upload(b"\xa5" * (16 * M)), ctx.upload(b"\xa5" * (32 * M))
    try:
        _check(ctx.lib.lh_debug_nova_fold(ctx.h, dim_vars, _fr_ptr(d["w1"]), _fr_ptr(d["w2"]), _fr_ptr(d_w), _fr_ptr(d.get("e1")),
                                          _fr_ptr(d["t"]), _fr_ptr(d.get("e2")), _fr_ptr(d_e), _fr_array([r])))
        out = frs_from_bytes(d_w.read()), frs_from_bytes(d_e.read())
    finally:
        for b in list(d.values()) + ([] if in_place else [d_w, d_e]):
            b.free()
    return out


# ------------------------------------------------------------------ batched Spartan, the verifier: several assignments of one key (tests/spartan_batch_ref.py)
def _batch_vars(count):
    return max((count - 1).bit_length(), 1)


def _spartan_batch_shape(num_vars, dim_vars, num_public, count):
    _spartan_shape(num_vars, dim_vars, num_public)
    if not (isinstance(count, int) and count >= 2):
        raise ArgumentError("spartan: num_instances out of range (at least 2)")
    if dim_vars + _batch_vars(count) > _ffi.LH_SPARTAN_BATCH_MAX_VARS:
        raise ArgumentError("spartan: dim_vars + batch_vars out of range (at most %d)" % _ffi.LH_SPARTAN_BATCH_MAX_VARS)


def _batch_publics(xs):
    xs = [list(x) for x in xs]
    if not xs or any(len(x) != len(xs[0]) for x in xs):
        raise ArgumentError("spartan: num_public public inputs for every instance")
    return xs, len(xs[0])


def spartan_verify_batch(vp, num_vars, dim_vars, commitment, xs, proof):
    """Verifier of a batched Spartan proof - len(xs) >= 2 assignments of one key in one proof, tests/spartan_batch_ref.py -
    (host only): `commitment` the bytes of R1csKey.commitment, `xs` the public inputs per instance, `proof` bytes or a
    transcript.  A Keccak256Transcript must be fully consumed."""
    if commitment is None or xs is None or proof is None:
        raise ArgumentError("spartan: null argument")
    xs, p = _batch_publics(xs)
    _spartan_batch_shape(num_vars, dim_vars, p, len(xs))
    t = Keccak256Transcript.from_proof(bytes(proof)) if isinstance(proof, (bytes, bytearray)) else proof
    _check(vp.lib.lh_spartan_verify_batch(vp.h, num_vars, dim_vars, _bytes_arg(commitment), len(commitment),
                                          _fr_array([v for x in xs for v in x]), len(xs), p, t.p))
    if isinstance(t, Keccak256Transcript) and t.remaining():
        raise InvalidSnark("spartan: trailing bytes in proof")


def verify_fractional_sum_check(num_vars, claimed_p_0s, claimed_q_0s, transcript):
    """fractional_sum_check.rs:193-270, the host verifier of prove_fractional_sum_check (a claim None: the root is read)
    -> (p_0s, q_0s, p_xs, q_xs, x): the roots come back because a caller checks a relation between them."""
    B = len(claimed_p_0s)
    if B != len(claimed_q_0s):
        raise ArgumentError("length mismatch")

    def opt(claims):
        keep = [_fr_array([c]) if c is not None else None for c in claims]
        arr = (C.POINTER(lh_fr) * max(B, 1))()
        for i, k in enumerate(keep):
            arr[i] = C.cast(k, C.POINTER(lh_fr)) if k is not None else None
        return arr, keep

    cp, keep_p = opt(claimed_p_0s)
    cq, keep_q = opt(claimed_q_0s)
    outs = [(lh_fr * max(B, 1))() for _ in range(4)]
    x = (lh_fr * max(num_vars, 1))()
    _check(_ffi.load().lh_gkr_fractional_verify(B, num_vars, cp, cq, transcript.p, *outs, x))
    return tuple(_fr_list(o, B) for o in outs) + (_fr_list(x, num_vars),)


def attach_comm(ctx, rank, size, all_gather, shard_bit):
    """Attach a caller-supplied communicator to the context (sharded proving): the transport of the
    CPU / one-GPU tests.  all_gather(send: bytes) -> bytes of size * len(send), rank-major; device-side gathers are
    staged through it.  A multi-GPU node uses attach_comm_rccl."""
    def cb(_user, send, recv, nbytes):
        try:
            out = all_gather(C.string_at(send, nbytes))
            if len(out) != nbytes * size:
                return _ffi.LH_ERR_ARG
            C.memmove(recv, out, len(out))
            return 0
        except Exception:  # the library turns this into an lh_status
            return _ffi.LH_ERR_DEVICE
    comm = _ffi.lh_comm()
    comm.rank, comm.size, comm.user = rank, size, None
    comm.all_gather = _ffi._AG_CB(cb)
    ctx._comm_keepalive = (comm, cb)
    _check(ctx.lib.lh_ctx_set_comm(ctx.h, C.byref(comm), shard_bit))


def rccl_unique_id():
    """ncclGetUniqueId: 128 bytes to hand to every rank's attach_comm_rccl (call on one rank)"""
    buf = C.create_string_buffer(_ffi.LH_RCCL_UNIQUE_ID_BYTES)
    _check(_ffi.load().lh_rccl_unique_id(buf))
    return buf.raw


def attach_comm_rccl(ctx, rank, size, unique_id, shard_bit):
    """RCCL communicator on the ctx's device and stream (collective over the `size` ranks): every exchange of a sharded
    proof is an ncclAllGather enqueued behind the kernels that produce its input."""
    if len(unique_id) != _ffi.LH_RCCL_UNIQUE_ID_BYTES:
        raise ArgumentError("unique id must be %d bytes" % _ffi.LH_RCCL_UNIQUE_ID_BYTES)
    _check(ctx.lib.lh_ctx_set_comm_rccl(ctx.h, rank, size, unique_id, shard_bit))


def comm_stats(ctx):
    """{"device": collectives issued on the device side (RCCL), "host": through the host callback}"""
    out = (C.c_uint64 * 2)()
    _check(ctx.lib.lh_ctx_comm_stats(ctx.h, out))
    return {"device": int(out[0]), "host": int(out[1])}


def comm_phase_stats(ctx, reset=False):
    """collectives and bytes (this rank's contribution) by phase of the Lasso prove that issued them"""
    out = (C.c_uint64 * 16)()
    _check(ctx.lib.lh_ctx_comm_phase_stats(ctx.h, out, 1 if reset else 0))
    names = ["witness", "commit", "surge", "leaves", "gkr", "evals", "open", "outside"]
    return {nm: {"collectives": int(out[2 * i]), "bytes": int(out[2 * i + 1])} for i, nm in enumerate(names) if out[2 * i]}


def memory_stats(ctx):
    """lh_ctx_memory_stats: the workspace arena's high-water mark and reservation, the device's free / total bytes"""
    out = (C.c_uint64 * 4)()
    _check(ctx.lib.lh_ctx_memory_stats(ctx.h, out))
    return {"arena_high_water_bytes": int(out[0]), "arena_reserved_bytes": int(out[1]), "device_free_bytes": int(out[2]),
            "device_total_bytes": int(out[3])}


def attach_comm_loopback(ctx, rank, size, shard_bit):
    """lh_ctx_set_comm_loopback: measurement aid - every peer is a copy of this rank (the transcript is not a valid proof)"""
    _check(ctx.lib.lh_ctx_set_comm_loopback(ctx.h, rank, size, shard_bit))


def detach_comm(ctx):
    _check(ctx.lib.lh_ctx_set_comm(ctx.h, None, 0))
    ctx._comm_keepalive = None


def shard_of(column, rank, size, shard_bit):
    """This rank's shard of a full column (numpy array of 2^n entries): entries whose index bits
    [shard_bit, shard_bit + log2 size) equal `rank`, in index order (local index hi || lo)."""
    rho = size.bit_length() - 1
    n = len(column)
    return column.reshape(n >> (shard_bit + rho), size, 1 << shard_bit)[:, rank, :].reshape(-1).copy()


def shard_poly(poly, rank, size, shard_bit):
    """This rank's shard of a device-resident MultilinearPolynomial (lh_shard_extract): a table of num_vars - rho variables"""
    rho = size.bit_length() - 1
    n_local = (1 << poly.num_vars) >> rho
    out = poly.ctx.alloc(32 * n_local)
    _check(poly.ctx.lib.lh_shard_extract(poly.ctx.h, poly.ptr, n_local, shard_bit, rho, rank, 32, out.ptr))
    return MultilinearPolynomial(poly.ctx, out, poly.num_vars - rho)


def lasso_prove_sharded(pp, table, num_vars, dims_local, transcript):
    """One proof over the ranks of the attached communicator; same bytes as lasso_prove.
    dims_local: THIS RANK'S shard of every chunk column (device u32[2^(num_vars - rho)], see shard_of)."""
    if len(dims_local) != table.c:
        raise ArgumentError("expected %d dim columns" % table.c)
    t = table.to_c()
    _check(pp.ctx.lib.lh_lasso_prove_sharded(pp.ctx.h, pp.h, C.byref(t), num_vars, _ptr_array(dims_local), transcript.p))


def lasso_last_timing(ctx):
    out = (C.c_double * _ffi.LH_LASSO_NUM_PHASES)()
    _check(ctx.lib.lh_lasso_last_timing(ctx.h, out))
    names = ["witness", "commit", "surge", "leaves", "gkr", "evals", "open_n", "open_l", "total"]
    return dict(zip(names, list(out)))


ROUTE_FIELDS = ["open_small_depth", "open_small_passes", "eq_factored_rounds", "standard_rounds", "rw_leaf_rounds",
                "resident_tails", "resident_rounds", "packed_ts_pairs", "derived_commitments", "sorted_dim_reuse",
                "sharded_rounds", "shard_exchanges", "window_table_jobs", "open_precommit", "resident_layers", "pp_folds", "msm_half_batches",
                "open_shared_sums", "open_precommit_staged"]


def lasso_last_route(ctx):
    """lh_lasso_last_route: which routes the last Lasso prove on `ctx` took (include/lasso_hip.h lh_lasso_route)"""
    out = (C.c_uint32 * 24)()
    _check(ctx.lib.lh_lasso_last_route(ctx.h, out))
    return dict(zip(ROUTE_FIELDS, [int(v) for v in out]))


def set_option(ctx, name, value):
    """lh_ctx_set_option: a route switch of the prover (include/lasso_hip.h lists them)"""
    _check(ctx.lib.lh_ctx_set_option(ctx.h, name.encode(), int(value)))


def get_option(ctx, name):
    out = C.c_int64(0)
    _check(ctx.lib.lh_ctx_get_option(ctx.h, name.encode(), C.byref(out)))
    return int(out.value)


def profile_enable(ctx, on=True):
    """lh_profile_enable: True / 1 = every instrumented launch synchronised (a separate, slower prove); 2 = live records of the
    bucket-accumulation launches only, nothing synchronised (usable inside a timed region); False / 0 = off"""
    _check(ctx.lib.lh_profile_enable(ctx.h, int(on)))


def profile_read(ctx):
    """-> list of dicts {name, ms, bytes, muls, items}, one per instrumented launch since enable."""
    n = C.c_size_t()
    _check(ctx.lib.lh_profile_read(ctx.h, None, 0, C.byref(n)))
    arr = (_ffi.lh_prof_rec * max(n.value, 1))()
    _check(ctx.lib.lh_profile_read(ctx.h, arr, n.value, C.byref(n)))
    return [dict(name=r.name.decode(), ms=r.ms, bytes=r.bytes, muls=r.muls, items=r.items) for r in arr[:n.value]]


from . import expression  # noqa: E402,F401  (host mirror of util::expression)
