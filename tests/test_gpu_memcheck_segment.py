"""GPU: memory checking in segments (hl.memcheck_prove_segment) - proof bytes against the golden proofs of the specification
(tests/memcheck_segment_ref.py, tests/golden/memcheck_segment.json), the host verifier and the commitments it returns, the
route switches, the final values on the device, the chain of three segments proved from hl.memcheck_replay's output, and
the refusals (the ctx goes on after each)."""
import array
import json
import os
import random

import pytest

import logup_gkr_ref as lgr
import memcheck_ref as mcr
import memcheck_segment_ref as msr

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FILE = json.load(open(os.path.join(HERE, "golden", "memcheck_segment.json")))
GOLDEN, CHAIN = FILE["cases"], FILE["chain"]
SS = [int(x, 16) for x in json.load(open(os.path.join(HERE, "golden", "lasso_tables.json")))["srs"]["ss"]]
SWITCHES = ["gkr_resident", "sc_tail", "sc_eq_factoring", "logup_fused_leaves"]


@pytest.fixture(scope="module")
def kzg6(hl, ctx):
    assert len(SS) == 6
    return hl.MultilinearKzg.setup(ctx, SS), hl.MultilinearKzgVerifierParams.setup(SS)


@pytest.fixture(scope="module")
def kzg14(hl, ctx):
    return hl.MultilinearKzg.setup(ctx, lgr.mid_ss()), hl.MultilinearKzgVerifierParams.setup(lgr.mid_ss())


_TRACES = {}


def _trace(case):
    """computed once per case and shared; callers copy before they damage a column"""
    if case not in _TRACES:
        _TRACES[case] = msr.case_trace(case)
    return _TRACES[case]


def _col(hl, ctx, words, vars_):
    return hl.U32Column(ctx.upload(array.array("I", words).tobytes()), vars_)


def _words(col):
    return array.array("I", col.buf.read()).tolist()


def _point(rec):
    return None if rec is None else (int(rec[0], 16), int(rec[1], 16))


def _prove(hl, ctx, pp, trace, l, image):
    """-> (proof, the final values read back)"""
    n = len(trace[0]).bit_length() - 1
    t = hl.Keccak256Transcript()
    final = hl.memcheck_prove_segment(pp, *[_col(hl, ctx, c, n) for c in trace], l, _col(hl, ctx, image, l), t)
    return t.into_proof(), _words(final)


def _prove_case(hl, ctx, pp, case):
    return _prove(hl, ctx, pp, _trace(case), msr.CASES[case][1], msr.case_image(case))


class _option:
    def __init__(self, hl, ctx, name, value):
        self.hl, self.ctx, self.name, self.value = hl, ctx, name, value

    def __enter__(self):
        self.old = self.hl.get_option(self.ctx, self.name)
        self.hl.set_option(self.ctx, self.name, self.value)

    def __exit__(self, *exc):
        self.hl.set_option(self.ctx, self.name, self.old)


# ------------------------------------------------------------------ 1. bytes, the verifier, the final values
@pytest.mark.parametrize("case", list(msr.CASES))
def test_proof_bytes_equal_the_golden_and_verify(hl, ctx, kzg6, kzg14, case):
    pp, vp = kzg6 if case in msr.SMALL else kzg14
    n, l = msr.CASES[case]
    proof, final = _prove_case(hl, ctx, pp, case)
    assert proof.hex() == GOLDEN[case]["proof"]
    t = hl.Keccak256Transcript.from_proof(proof)
    iv_c, fv_c = hl.memcheck_verify_segment(vp, n, l, t)
    assert t.remaining() == 0
    assert (iv_c, fv_c) == (_point(GOLDEN[case]["image_commitment"]), _point(GOLDEN[case]["final_commitment"]))
    # d_final is the specification's fv
    assert final == mcr.witness(*_trace(case), msr.case_image(case))["fv"]
    if case == "zero_image":  # iv commits to the identity: bit 3 of the mask (its repr is big-endian)
        assert int.from_bytes(proof[:32], "big") == 1 << msr.IV and iv_c is None


@pytest.mark.parametrize("case", ["small_mem", "mid"])
def test_bytes_do_not_depend_on_the_switches(hl, ctx, kzg6, kzg14, case):
    pp, _ = kzg6 if case in msr.SMALL else kzg14
    for name in SWITCHES:
        with _option(hl, ctx, name, 0):
            assert _prove_case(hl, ctx, pp, case)[0].hex() == GOLDEN[case]["proof"], name + " = 0"


# ------------------------------------------------------------------ 2. the chain, on the device from end to end
def test_the_chain_is_proved_from_the_replay_and_verifies(hl, ctx, kzg6):
    pp, vp = kzg6
    n, l, count = msr.CHAIN
    image = _col(hl, ctx, msr.chain_image(), l)
    _, images = msr.chain_traces()
    proofs = []
    for k in range(count):
        addr, store, val = [_col(hl, ctx, c, n) for c in msr.chain_ops(k)]
        rv, wv, replayed = hl.memcheck_replay(ctx, addr, store, val, l, image=image)
        t = hl.Keccak256Transcript()
        final = hl.memcheck_prove_segment(pp, addr, rv, wv, l, image, t)  # (from the previous d_final: no host trip)
        proofs.append(t.into_proof())
        assert proofs[-1].hex() == CHAIN[k]["proof"], "segment %d" % k
        assert _words(final) == _words(replayed) == images[k + 1]
        image = final
    first, last = hl.memcheck_verify_chain(vp, l, [(n, p) for p in proofs])
    assert (first, last) == (_point(CHAIN[0]["image_commitment"]), _point(CHAIN[2]["final_commitment"]))
    with pytest.raises(hl.InvalidSnark, match="memcheck chain: segment 1 does not start where segment 0 ends"):
        hl.memcheck_verify_chain(vp, l, [(n, proofs[0]), (n, proofs[2]), (n, proofs[1])])


def test_final_goes_where_the_caller_says(hl, ctx, kzg6):
    pp, _ = kzg6
    n, l = msr.CASES["small_mem"]
    out = hl.U32Column(ctx.alloc(4 << l), l)
    t = hl.Keccak256Transcript()
    got = hl.memcheck_prove_segment(pp, *[_col(hl, ctx, c, n) for c in _trace("small_mem")], l,
                                    _col(hl, ctx, msr.case_image("small_mem"), l), t, final=out)
    assert got is out and t.into_proof().hex() == GOLDEN["small_mem"]["proof"]
    fv = mcr.witness(*_trace("small_mem"), msr.case_image("small_mem"))["fv"]
    assert _words(out) == fv
    # the image's own memory may take the final values: it is overwritten behind the proof's last read of it
    image = _col(hl, ctx, msr.case_image("small_mem"), l)
    t = hl.Keccak256Transcript()
    hl.memcheck_prove_segment(pp, *[_col(hl, ctx, c, n) for c in _trace("small_mem")], l, image, t, final=image)
    assert t.into_proof().hex() == GOLDEN["small_mem"]["proof"] and _words(image) == fv != msr.case_image("small_mem")


# ------------------------------------------------------------------ 3. refusals, and the ctx afterwards
def test_an_inconsistent_rv_is_refused_and_the_ctx_goes_on(hl, ctx, kzg6, kzg14):
    pp6, _ = kzg6
    pp, _ = kzg14
    n, l = msr.CASES["mid"]
    image = msr.case_image("mid")
    addr, rv, wv = _trace("mid")
    for at in (0, (1 << n) // 2 + 77, (1 << n) - 1):  # first, middle, last operation
        bad = list(rv)
        bad[at] ^= 0x10000
        t = hl.Keccak256Transcript()
        with pytest.raises(hl.InvalidSnark, match="Invalid memory trace"):
            hl.memcheck_prove_segment(pp, *[_col(hl, ctx, c, n) for c in (addr, bad, wv)], l, _col(hl, ctx, image, l), t)
        assert not t.into_proof(), "refused before a byte is written"
        assert _prove_case(hl, ctx, pp6, "one_var")[0].hex() == GOLDEN["one_var"]["proof"]


def test_nv_above_the_srs_is_refused(hl, ctx, kzg6):
    pp, _ = kzg6
    rng = random.Random(7)
    trace = mcr.trace_of([(rng.randrange(8), rng.randrange(1 << 32)) for _ in range(1 << 7)], [0] * 8)
    with pytest.raises(hl.InvalidPcsParam):  # seven variables of operations against the six of the SRS
        hl.memcheck_prove_segment(pp, *[_col(hl, ctx, c, 7) for c in trace], 3, _col(hl, ctx, [0] * 8, 3), hl.Keccak256Transcript())
    small = [_col(hl, ctx, c, 5) for c in _trace("small_mem")]
    with pytest.raises(hl.InvalidPcsParam):  # the memory's seven variables are above it too
        hl.memcheck_prove_segment(pp, *small, 7, _col(hl, ctx, [0] * 128, 7), hl.Keccak256Transcript())
    assert _prove_case(hl, ctx, pp, "one_var")[0].hex() == GOLDEN["one_var"]["proof"]
