"""GPU: the read-write memory-checking argument (hl.memcheck_prove) - proof bytes against the golden proofs of the
specification (tests/memcheck_ref.py, tests/golden/memcheck.json), the host verifier, the route switches, the launch records
of its four kernels, refusals (the ctx goes on after each), and a size at which every kernel runs many workgroups (n = 16,
no Python reference: the host verifier is the check)."""
import array
import ctypes as C
import json
import os
import random

import pytest

import logup_gkr_ref as lgr
import memcheck_ref as mcr
from oracle.pyref.field import R_MOD as P

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "memcheck.json")))["cases"]
SS = [int(x, 16) for x in json.load(open(os.path.join(HERE, "golden", "lasso_tables.json")))["srs"]["ss"]]
SWITCHES = ["gkr_resident", "sc_tail", "sc_eq_factoring", "logup_fused_leaves"]
LARGE = (16, 10)


@pytest.fixture(scope="module")
def kzg6(hl, ctx):
    assert len(SS) == 6
    return hl.MultilinearKzg.setup(ctx, SS), hl.MultilinearKzgVerifierParams.setup(SS)


@pytest.fixture(scope="module")
def kzg16(hl, ctx):
    """sixteen variables whose first fourteen secrets are `mid`'s: a level depends on the secrets below it alone"""
    rng = random.Random(lgr.MID_SRS_SEED + 1)
    ss = lgr.mid_ss() + [rng.randrange(1, P) for _ in range(2)]
    return hl.MultilinearKzg.setup(ctx, ss), hl.MultilinearKzgVerifierParams.setup(ss)


_TRACES = {}


def _trace(case):
    """computed once per case and shared; callers copy before they damage a column"""
    if case not in _TRACES:
        _TRACES[case] = mcr.case_trace(case)
    return _TRACES[case]


def _upload(hl, ctx, cols, n):
    return [hl.U32Column(ctx.upload(array.array("I", c).tobytes()), n) for c in cols]


def _prove(hl, ctx, pp, trace, l, init):
    n = len(trace[0]).bit_length() - 1
    t = hl.Keccak256Transcript()
    hl.memcheck_prove(pp, *_upload(hl, ctx, trace, n), l, t, init=init)
    return t.into_proof()


def _prove_case(hl, ctx, pp, case):
    return _prove(hl, ctx, pp, _trace(case), mcr.CASES[case][1], mcr.case_init(case))


def _profiled(hl, ctx, fn):
    hl.profile_enable(ctx, True)
    try:
        out = fn()
        return out, hl.profile_read(ctx)
    finally:
        hl.profile_enable(ctx, False)


class _option:
    def __init__(self, hl, ctx, name, value):
        self.hl, self.ctx, self.name, self.value = hl, ctx, name, value

    def __enter__(self):
        self.old = self.hl.get_option(self.ctx, self.name)
        self.hl.set_option(self.ctx, self.name, self.value)

    def __exit__(self, *exc):
        self.hl.set_option(self.ctx, self.name, self.old)


# ------------------------------------------------------------------ 1. bytes and the verifier
@pytest.mark.parametrize("case", list(mcr.CASES))
def test_proof_bytes_equal_the_golden_and_verify(hl, ctx, kzg6, kzg16, case):
    pp, vp = kzg6 if case in mcr.SMALL else kzg16
    n, l, _ = mcr.CASES[case]
    proof = _prove_case(hl, ctx, pp, case)
    assert proof.hex() == GOLDEN[case]["proof"]
    t = hl.Keccak256Transcript.from_proof(proof)
    hl.memcheck_verify(vp, n, l, t, init=mcr.case_init(case))
    assert t.remaining() == 0
    if case == "distinct":  # rt is the zero column and commits to the identity: bit 3 of the mask (its repr is big-endian)
        assert int.from_bytes(proof[:32], "big") == 1 << 3


# ------------------------------------------------------------------ 2. the route switches: same bytes
@pytest.mark.parametrize("case", ["small_mem", "mid"])
def test_bytes_do_not_depend_on_the_switches(hl, ctx, kzg6, kzg16, case):
    pp, _ = kzg6 if case in mcr.SMALL else kzg16
    assert hl.get_option(ctx, "logup_fused_leaves") in (0, 1)
    for name in SWITCHES:
        with _option(hl, ctx, name, 0):
            assert _prove_case(hl, ctx, pp, case).hex() == GOLDEN[case]["proof"], name + " = 0"
    with _option(hl, ctx, "logup_fused_leaves", 1):
        assert _prove_case(hl, ctx, pp, case).hex() == GOLDEN[case]["proof"]


# ------------------------------------------------------------------ 3. launch records
@pytest.mark.parametrize("case", ["small_mem", "mid", "wide"])  # (wide: the level above comes with the cells' leaves alone)
def test_launch_records(hl, ctx, kzg6, kzg16, case):
    pp, _ = kzg6 if case in mcr.SMALL else kzg16
    n, l, _ = mcr.CASES[case]
    N, M = 1 << n, 1 << l
    for fused in (1, 0):
        with _option(hl, ctx, "logup_fused_leaves", fused):
            proof, recs = _profiled(hl, ctx, lambda: _prove_case(hl, ctx, pp, case))
        assert proof.hex() == GOLDEN[case]["proof"]
        by = {}
        for r in recs:
            by.setdefault(r["name"], []).append(r)
        # one launch each, once per proof: the witness, the multiplicities, the four trees' leaves, the two fractions' leaves
        assert [r["items"] for r in by["memcheck_trace"]] == [N] and by["memcheck_trace"][0]["bytes"] == 36 * N + 16 * M
        assert [r["items"] for r in by["memcheck_m"]] == [N] and by["memcheck_m"][0]["bytes"] == 12 * N
        assert [r["items"] for r in by["memcheck_leaves"]] == [N + M]
        assert [r["items"] for r in by["memcheck_range_leaves"]] == [N]
        # an operation reads its four words, a cell its three; two 32-byte leaves each; with the level above 32 bytes more
        up_n, up_l = fused and n >= 12, fused and l >= 12
        assert by["memcheck_leaves"][0]["bytes"] == (16 + 64 + 32 * up_n) * N + (12 + 64 + 32 * up_l) * M
        assert by["memcheck_range_leaves"][0]["bytes"] == (8 + 4 * 32 + (2 * 32 if fused else 0)) * N
        # the fractions' level above the leaves comes with them or from frac_up: one record per fraction and level
        assert len(by.get("frac_up", [])) == 2 * (n - 2 if fused else n - 1)
        # nothing of the lookup arguments runs here
        assert not any(name.startswith(("logup_", "lasso_")) for name in by)


# ------------------------------------------------------------------ 4. refusals, and the ctx afterwards
def test_invalid_traces_are_invalid_snark_and_the_ctx_goes_on(hl, ctx, kzg6, kzg16):
    pp6, _ = kzg6
    pp, _ = kzg16
    n, l, _ = mcr.CASES["mid"]
    init = mcr.case_init("mid")
    addr, rv, wv = _trace("mid")

    def refused(a, r, w):
        t = hl.Keccak256Transcript()
        with pytest.raises(hl.InvalidSnark, match="Invalid memory trace"):
            hl.memcheck_prove(pp, *_upload(hl, ctx, (a, r, w), n), l, t, init=init)
        assert not t.into_proof(), "refused before a byte is written"
        assert _prove_case(hl, ctx, pp6, "one_var").hex() == GOLDEN["one_var"]["proof"]

    for at in (0, (1 << n) // 2 + 77, (1 << n) - 1):  # an rv that is not the last value written: first, middle, last operation
        bad = list(rv)
        bad[at] ^= 0x10000
        refused(addr, bad, wv)
    for at, a in ((5, 1 << l), ((1 << n) - 1, (1 << 31) | addr[-1])):  # an address outside the memory, low bits in range or not
        bad = list(addr)
        bad[at] = a
        refused(bad, rv, wv)
    # a store whose wv nobody reads back wrongly is fine: the last operation's wv is free
    free = list(wv)
    free[-1] ^= 1
    assert _prove(hl, ctx, pp, (addr, rv, free), l, init) != bytes.fromhex(GOLDEN["mid"]["proof"])


def test_refusals_on_the_device_side(hl, ctx, kzg6):
    from halo2_lasso_amd import _ffi
    pp, _ = kzg6
    lib = ctx.lib
    good = lambda: _prove_case(hl, ctx, pp, "one_var").hex() == GOLDEN["one_var"]["proof"]
    rng = random.Random(7)
    n = 7
    cols = _upload(hl, ctx, mcr.trace_of([(rng.randrange(8), rng.randrange(1 << 32)) for _ in range(1 << n)], [0] * 8), n)
    with pytest.raises(hl.InvalidPcsParam):  # nv = 7 above the six variables of the SRS
        hl.memcheck_prove(pp, *cols, 3, hl.Keccak256Transcript())
    assert good()
    small = _upload(hl, ctx, _trace("small_mem"), 5)
    with pytest.raises(hl.InvalidPcsParam):  # the memory's 7 variables are above it too
        hl.memcheck_prove(pp, *small, 7, hl.Keccak256Transcript())
    assert good()
    trace = _ffi.lh_memcheck_trace()
    trace.d_addr, trace.d_rv, trace.d_wv = [C.cast(C.c_void_p(c.ptr), C.POINTER(C.c_uint32)) for c in small]
    image = (C.c_uint32 * 8)(*mcr.case_init("small_mem"))
    t = hl.Keccak256Transcript()
    # 25 variables of memory with an image (the verifier would fold 2^25 words): refused on entry, the image is not read
    assert lib.lh_memcheck_prove(ctx.h, pp.h, C.byref(trace), 5, 25, image, t.p) == _ffi.LH_ERR_ARG
    assert b"mem_vars" in lib.lh_last_error() and good()
    assert lib.lh_memcheck_prove(ctx.h, None, C.byref(trace), 5, 3, image, t.p) == _ffi.LH_ERR_ARG  # NULL SRS
    assert lib.lh_memcheck_prove(ctx.h, pp.h, None, 5, 3, image, t.p) == _ffi.LH_ERR_ARG  # NULL trace
    assert lib.lh_memcheck_prove(ctx.h, pp.h, C.byref(trace), 5, 3, image, None) == _ffi.LH_ERR_ARG  # NULL transcript
    assert lib.lh_memcheck_prove(ctx.h, pp.h, C.byref(trace), 0, 3, image, t.p) == _ffi.LH_ERR_ARG
    holed = _ffi.lh_memcheck_trace()
    holed.d_addr, holed.d_wv = trace.d_addr, trace.d_wv
    assert lib.lh_memcheck_prove(ctx.h, pp.h, C.byref(holed), 5, 3, image, t.p) == _ffi.LH_ERR_ARG  # a NULL column
    assert b"d_rv" in lib.lh_last_error() and not t.into_proof(), "refused before a byte is written"
    assert lib.lh_memcheck_prove(ctx.h, pp.h, C.byref(trace), 5, 3, image, t.p) == _ffi.LH_OK
    assert t.into_proof().hex() == GOLDEN["small_mem"]["proof"]
    # the image is part of the statement: without it this trace does not start from zeros
    with pytest.raises(hl.InvalidSnark, match="Invalid memory trace"):
        hl.memcheck_prove(pp, *small, 3, hl.Keccak256Transcript())
    assert good()


# ------------------------------------------------------------------ 5. a size with many workgroups in every kernel
def test_larger_shape_round_trips(hl, ctx, kzg16):
    pp, vp = kzg16
    n, l = LARGE
    rng = random.Random(1610)
    init = [rng.randrange(1 << 32) for _ in range(1 << l)]
    ops = [(rng.randrange(1 << l), rng.randrange(1 << 32) if rng.randrange(2) else None) for _ in range(1 << n)]
    trace = mcr.trace_of(ops, init)
    proofs = []
    for fused in (1, 0):
        with _option(hl, ctx, "logup_fused_leaves", fused):
            proofs.append(_prove(hl, ctx, pp, trace, l, init))
    assert proofs[0] == proofs[1]
    t = hl.Keccak256Transcript.from_proof(proofs[0])
    hl.memcheck_verify(vp, n, l, t, init=init)
    assert t.remaining() == 0
    changed = list(init)
    changed[513] ^= 1
    with pytest.raises(hl.InvalidSnark):
        hl.memcheck_verify(vp, n, l, hl.Keccak256Transcript.from_proof(proofs[0]), init=changed)
