"""GPU: Nova folding and relaxed Spartan (hl.nova_instance / hl.nova_fold / hl.spartan_prove_relaxed) - instance blobs, fold
proofs and relaxed proofs against the golden file of the specification (tests/nova_ref.py, tests/golden/nova.json), the
folded vectors read back, their commitments, folding in place, the two groupings of a chain, the launch records of a fold,
the route switches, inputs that do not satisfy their relation, refusals (the ctx goes on after each), and the plain prover's
bytes after folds on the same ctx and key."""
import array
import ctypes as C
import hashlib
import json
import os
import random
import types

import pytest

import logup_gkr_ref as lgr
import nova_ref as nv
import spartan_ref as spa
from oracle.pyref.field import R_MOD as P
from oracle.pyref.transcript import Keccak256Transcript as OT

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "nova.json")))["cases"]
SPARTAN_GOLDEN = json.load(open(os.path.join(HERE, "golden", "spartan.json")))["cases"]
SS = [int(x, 16) for x in json.load(open(os.path.join(HERE, "golden", "lasso_tables.json")))["srs"]["ss"]]
SWITCHES = ["gkr_resident", "sc_tail", "sc_eq_factoring"]


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


def _commit(hl, ctx, pp, inst, l):
    n = len(inst[0][2]).bit_length() - 1
    up = lambda col: hl.U32Column(ctx.upload(array.array("I", col).tobytes()), n)
    return hl.r1cs_commit(ctx, pp, [(up(row), up(col), hl.MultilinearPolynomial.new(ctx, val)) for row, col, val in inst], l)


def _commit_case(hl, ctx, pp, case):
    return _commit(hl, ctx, pp, nv.case_instance(case)[0], nv.CASES[case][1])


def _sparse_key(case):
    """what nova_ref's witness half needs of a key: the entries, no commitment"""
    n, l, _ = nv.CASES[case]
    return types.SimpleNamespace(n=n, l=l, mats=[types.SimpleNamespace(dims=[row, col], val=val) for row, col, val in nv.case_instance(case)[0]])


def _is(rec, part, data):
    """the bytes are the golden ones: pinned by length and SHA-256, `mid` in full"""
    return (len(data), hashlib.sha256(data).hexdigest()) == (rec[part + "_bytes"], rec[part + "_sha256"]) and \
        data.hex() == rec.get(part, data.hex())


def _vector(hl, ctx, vars_):
    return hl.MultilinearPolynomial(ctx, ctx.alloc(32 << vars_), vars_)


def run_device(hl, ctx, pp, key, case, schedule=None, in_place=False, prove=True):
    """nova_ref.run on the device -> (slots, records): slots[i] = (blob, d_w, d_e or None).  in_place: a fold whose first
    input is itself folded writes into that input's vectors."""
    l = key.dim_vars
    assigns = nv.case_instance(case)[1]
    slots, records = [], []
    for step in (nv.SCHEDULES[case] if schedule is None else schedule):
        if step[0] == "fresh":
            w, x = assigns[step[1]]
            d_w = hl.MultilinearPolynomial.new(ctx, w)
            blob = hl.nova_instance(ctx, pp, key, d_w, x)
            slots.append((blob, d_w, None))
            records.append({"step": "fresh", "blob": blob})
        elif step[0] == "fold":
            (b1, w1, e1), (b2, w2, e2) = slots[step[1]], slots[step[2]]
            w_out, e_out = (w1, e1) if in_place and e1 is not None else (_vector(hl, ctx, l - 1), _vector(hl, ctx, l))
            blob, proof = hl.nova_fold(ctx, pp, key, b1, w1, e1, b2, w2, e2, w_out, e_out)
            slots.append((blob, w_out, e_out))
            records.append({"step": "fold", "a": step[1], "b": step[2], "proof": proof, "blob": blob})
        elif prove:
            blob, d_w, d_e = slots[step[1]]
            records.append({"step": "prove", "a": step[1], "proof": hl.spartan_prove_relaxed(ctx, pp, key, blob, d_w, d_e)})
    return slots, records


def _golden_records(case, records):
    want = [s for s in GOLDEN[case]["steps"]][:len(records)]
    return len(want) == len(records) and all(
        _is(s, part, rec[part]) for rec, s in zip(records, want) for part in ("blob", "proof") if part in rec)


def _tiny_still_proves(hl, ctx, pp):
    with _commit_case(hl, ctx, pp, "tiny") as key:
        return _golden_records("tiny", run_device(hl, ctx, pp, key, "tiny")[1])


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


def _spec_vectors(case, records):
    """the folded (w, E) of every slot by the specification's witness half, with r read off the golden fold proofs by the
    specification's fold verifier: big integers, no commitment"""
    key = _sparse_key(case)
    assigns = nv.case_instance(case)[1]
    out = []
    for step, rec in zip(nv.SCHEDULES[case], records):
        if rec["step"] == "fresh":
            w, x = assigns[step[1]]
            out.append((nv.Instance(None, None, x), (w, None)))
        elif rec["step"] == "fold":
            (U1, W1), (U2, W2) = out[rec["a"]], out[rec["b"]]
            T = nv.cross_term(key, U1, W1, U2, W2)
            r = rec["r"]
            out.append((nv.Instance(None, None, [(a + r * b) % P for a, b in zip(U1.x, U2.x)]), nv.fold_witness(W1, W2, T, r)))
    return out


def _challenges(case, key_blob, records):
    """records with the challenge r of every fold, from the specification's fold verifier on the device's bytes"""
    n, l, p = nv.CASES[case]
    blobs = [r["blob"] for r in records if r["step"] != "prove"]
    for rec in records:
        if rec["step"] == "fold":
            got = []
            assert nv.fold_verify(n, l, p, key_blob, blobs[rec["a"]], blobs[rec["b"]], OT(rec["proof"]), challenge=got) == rec["blob"]
            rec["r"] = got[0]
    return records


# ------------------------------------------------------------------ 1. bytes, the verifiers, the vectors, their commitments
@pytest.mark.parametrize("case", list(nv.CASES))
def test_bytes_equal_the_golden_and_verify(hl, ctx, kzg6, kzg16, case):
    pp, vp = kzg6 if case in nv.SMALL else kzg16
    n, l, p = nv.CASES[case]
    with _commit_case(hl, ctx, pp, case) as key:
        assert _is(GOLDEN[case], "key", key.commitment)
        slots, records = run_device(hl, ctx, pp, key, case)
        assert _golden_records(case, records) and len(records) == len(GOLDEN[case]["steps"])
        blobs = [r["blob"] for r in records if r["step"] != "prove"]
        for rec in records:
            if rec["step"] == "fold":
                assert hl.nova_fold_verify(n, l, key.commitment, blobs[rec["a"]], blobs[rec["b"]], rec["proof"]) == rec["blob"]
            if rec["step"] == "prove":
                hl.spartan_verify_relaxed(vp, n, l, key.commitment, blobs[rec["a"]], p, rec["proof"])
        # the folded w and E, read back, are the specification's; batch_commit of them gives the folded commitments
        spec = _spec_vectors(case, _challenges(case, key.commitment, records))
        ident = lambda pt: None if pt is None or tuple(pt) == (0, 0) else tuple(pt)
        for (blob, d_w, d_e), (U, (w, E)) in zip(slots, spec):
            assert d_w.evals() == w and (d_e is None) == (E is None)
            if d_e is not None:
                assert d_e.evals() == E
            cw = ident(hl.MultilinearKzg.commit(pp, d_w))
            ce = ident(hl.MultilinearKzg.commit(pp, d_e)) if d_e is not None else None
            assert nv.Instance(cw, ce, U.x).blob == blob


def test_folding_in_place_gives_the_same_bytes(hl, ctx, kzg6):
    pp, vp = kzg6
    for case in ("chain", "two_relaxed"):
        with _commit_case(hl, ctx, pp, case) as key:
            slots, records = run_device(hl, ctx, pp, key, case, in_place=True)
            assert _golden_records(case, records)
            # chain's second and third fold wrote into the first fold's vectors: one accumulator
            if case == "chain":
                assert slots[5][1] is slots[4][1] and slots[6][2] is slots[4][2]


def test_a_chain_folds_in_either_grouping(hl, ctx, kzg6):
    pp, vp = kzg6
    case = "chain"
    n, l, p = nv.CASES[case]
    fresh = [("fresh", k) for k in range(4)]
    left = fresh + [("fold", 0, 1), ("fold", 4, 2), ("fold", 5, 3), ("prove", 6)]  # ((0 1) 2) 3: the golden one
    right = fresh + [("fold", 2, 3), ("fold", 1, 4), ("fold", 0, 5), ("prove", 6)]  # 0 (1 (2 3)): every second input is folded
    with _commit_case(hl, ctx, pp, case) as key:
        proofs = []
        for schedule in (left, right):
            slots, records = run_device(hl, ctx, pp, key, case, schedule=schedule)
            blobs = [r["blob"] for r in records if r["step"] != "prove"]
            for rec in records:
                if rec["step"] == "fold":
                    assert hl.nova_fold_verify(n, l, key.commitment, blobs[rec["a"]], blobs[rec["b"]], rec["proof"]) == rec["blob"]
            hl.spartan_verify_relaxed(vp, n, l, key.commitment, blobs[6], p, records[-1]["proof"])
            proofs.append((blobs[6], records[-1]["proof"]))
        assert left == nv.SCHEDULES[case] and proofs[0][0] != proofs[1][0] and proofs[0][1] != proofs[1][1]
        with pytest.raises(hl.InvalidSnark):  # one grouping's proof against the other's instance
            hl.spartan_verify_relaxed(vp, n, l, key.commitment, proofs[0][0], p, proofs[1][1])


# ------------------------------------------------------------------ 2. launch records of a fold
@pytest.mark.parametrize("case", ["chain", "mid"])
def test_launch_records_of_a_fold(hl, ctx, kzg6, kzg16, case):
    pp, _ = kzg6 if case in nv.SMALL else kzg16
    n, l, p = nv.CASES[case]
    N, M = 1 << n, 1 << l
    with _commit_case(hl, ctx, pp, case) as key:
        slots, _ = run_device(hl, ctx, pp, key, case, prove=False)
        fold = [s for s in nv.SCHEDULES[case] if s[0] == "fold"][-1]  # a folded first input, a fresh second one
        (b1, w1, e1), (b2, w2, e2) = slots[fold[1]], slots[fold[2]]
        assert e1 is not None and e2 is None
        w_out, e_out = _vector(hl, ctx, l - 1), _vector(hl, ctx, l)
        (blob, proof), recs = _profiled(hl, ctx, lambda: hl.nova_fold(ctx, pp, key, b1, w1, e1, b2, w2, e2, w_out, e_out))
        assert blob == slots[-1][0]
        by = {}
        for r in recs:
            by.setdefault(r["name"], []).append(r)
        assert [(r["items"], r["muls"], r["bytes"]) for r in by["nova_spmv2"]] == [(3 * N, 6 * N, 3 * (108 * N + 64 * M))]
        # the cross term: six products, E1 and T; eight field products a row
        assert [(r["items"], r["muls"], r["bytes"]) for r in by["nova_cross_term"]] == [(M, 8 * M, 32 * M * 8)]
        # the commitment of T: one MSM batch of 2^l full-width scalars
        assert [(r["items"], r["muls"]) for r in by["msm_digits"]] == [(M, M)]
        assert [(r["items"], r["muls"], r["bytes"]) for r in by["nova_fold"]] == [(M // 2 + M, M // 2 + M, 96 * (M // 2) + 32 * M * 3)]
        # no sort of the key's kind, no counter, no Spark kernel, no plain keyed sum, no sum-check round
        names = [r["name"] for r in recs]
        assert not any(name.startswith(("spark_", "spartan_", "lasso_counters", "sum_check", "sc_", "gkr_")) for name in names), names
        order = [name for name in names if name.startswith("nova_") or name == "msm_digits"]
        assert order == ["nova_spmv2", "nova_cross_term", "msm_digits", "nova_fold"]


# ------------------------------------------------------------------ 3. the route switches: same bytes
@pytest.mark.parametrize("case", ["chain", "mid"])
def test_bytes_do_not_depend_on_the_switches(hl, ctx, kzg6, kzg16, case):
    pp, _ = kzg6 if case in nv.SMALL else kzg16
    with _commit_case(hl, ctx, pp, case) as key:
        slots, records = run_device(hl, ctx, pp, key, case, prove=False)
        assert _golden_records(case, records)
        blob, d_w, d_e = slots[-1]
        want = GOLDEN[case]["steps"][-1]
        for name in SWITCHES:
            with _option(hl, ctx, name, 0):
                assert _is(want, "proof", hl.spartan_prove_relaxed(ctx, pp, key, blob, d_w, d_e)), name + " = 0"
                assert _golden_records(case, run_device(hl, ctx, pp, key, case, prove=False)[1]), name + " = 0"


# ------------------------------------------------------------------ 4. inputs that do not satisfy, refusals, the ctx afterwards
def test_an_unsatisfying_input_is_refused_before_the_transcript(hl, ctx, kzg6):
    pp, _ = kzg6
    case = "two_relaxed"
    n, l, p = nv.CASES[case]
    inst, assigns = nv.case_instance(case)
    with _commit_case(hl, ctx, pp, case) as key:
        slots, records = run_device(hl, ctx, pp, key, case, prove=False)
        spec = _spec_vectors(case, _challenges(case, key.commitment, records))
        (b1, w1, e1), (b2, w2, e2) = slots[4], slots[5]
        (U1, (sw1, sE1)), (U2, (sw2, sE2)) = spec[4], spec[5]
        outs = lambda: (_vector(hl, ctx, l - 1), _vector(hl, ctx, l))

        def refused(words, *args):
            t = hl.Keccak256Transcript()
            with pytest.raises(hl.ArgumentError, match=words):
                hl.nova_fold(ctx, pp, key, *args, *outs(), transcript=t)
            assert not t.into_proof(), "nothing was written"

        # one element of w1: the count is the dense statement's
        bad_w = list(sw1)
        bad_w[0] = (bad_w[0] + 1) % P
        count = nv.relaxed_satisfied(inst, bad_w, sE1, U1.x, l)
        assert count >= 1
        refused(r"nova: input 1 does not satisfy %d of the 2\^3 constraints" % count,
                b1, hl.MultilinearPolynomial.new(ctx, bad_w), e1, b2, w2, e2)
        # one element of E2
        bad_e = list(sE2)
        bad_e[5] = (bad_e[5] + 1) % P
        assert nv.relaxed_satisfied(inst, sw2, bad_e, U2.x, l) == 1
        refused(r"nova: input 2 does not satisfy 1 of the 2\^3 constraints", b1, w1, e1, b2, w2, hl.MultilinearPolynomial.new(ctx, bad_e))
        # another x: the blob of input 2 with x[1] + 1 (u = x[0] is as it was)
        other = nv.read_instance(b2, p)
        other.x[1] = (other.x[1] + 1) % P
        count = nv.relaxed_satisfied(inst, sw2, sE2, other.x, l)
        assert count >= 1
        refused(r"nova: input 2 does not satisfy %d of the 2\^3 constraints" % count, b1, w1, e1, other.blob, w2, e2)
        # a fresh witness that does not satisfy: no instance
        w, x = assigns[0]
        with pytest.raises(hl.ArgumentError, match=r"nova: the witness does not satisfy \d of the 2\^3 constraints"):
            hl.nova_instance(ctx, pp, key, hl.MultilinearPolynomial.new(ctx, [(v + 1) % P for v in w]), x)
        with pytest.raises(hl.ArgumentError, match=r"nova: a fresh instance has x\[0\] = 1"):
            hl.nova_instance(ctx, pp, key, hl.MultilinearPolynomial.new(ctx, w), [2] + x[1:])
        # the relaxed prover: a damaged E
        t = hl.Keccak256Transcript()
        with pytest.raises(hl.ArgumentError, match=r"spartan: the witness does not satisfy 1 of the 2\^3 constraints"):
            hl.spartan_prove_relaxed(ctx, pp, key, b2, w2, hl.MultilinearPolynomial.new(ctx, bad_e), transcript=t)
        assert not t.into_proof()
        # ... and an E that is not zero beside a C_E that is the identity (a fresh instance's blob): before the transcript too
        b0, w0, _ = slots[0]
        t = hl.Keccak256Transcript()
        with pytest.raises(hl.ArgumentError, match="spartan: the instance's C_E is the identity but E is not zero"):
            hl.spartan_prove_relaxed(ctx, pp, key, b0, w0, hl.MultilinearPolynomial.new(ctx, [0] * 7 + [1]), transcript=t)
        assert not t.into_proof()
        zero_e = hl.MultilinearPolynomial.new(ctx, [0] * 8)  # (a zero vector is as good as none)
        assert hl.spartan_prove_relaxed(ctx, pp, key, b0, w0, zero_e) == hl.spartan_prove_relaxed(ctx, pp, key, b0, w0, None)
        # the honest fold goes through afterwards, with the golden bytes
        blob, proof = hl.nova_fold(ctx, pp, key, b1, w1, e1, b2, w2, e2, *outs())
        assert _is(GOLDEN[case]["steps"][6], "blob", blob) and _is(GOLDEN[case]["steps"][6], "proof", proof)
    assert _tiny_still_proves(hl, ctx, pp)


def test_refusals_and_the_ctx_goes_on(hl, ctx, kzg6):
    from halo2_lasso_amd import _ffi
    pp, vp = kzg6
    lib = ctx.lib
    good = lambda: _tiny_still_proves(hl, ctx, pp)
    case = "chain"
    n, l, p = nv.CASES[case]
    key = _commit_case(hl, ctx, pp, case)
    slots, records = run_device(hl, ctx, pp, key, case, prove=False)
    (b1, w1, e1), (b2, w2, e2) = slots[4], slots[2]
    outs = lambda: (_vector(hl, ctx, l - 1), _vector(hl, ctx, l))
    fold = lambda *a: hl.nova_fold(ctx, pp, key, *a, *outs())
    # blobs of the wrong length, with a mask out of range; two instances with a different p
    for bad in (b1[:-1], b1 + b"\0", b"\0" * 31 + b"\x04" + b1[32:], b"\1", b""):
        with pytest.raises(hl.ArgumentError, match="nova: malformed instance"):
            fold(bad, w1, e1, b2, w2, e2)
        with pytest.raises(hl.ArgumentError, match="nova: malformed instance"):
            fold(b2, w2, e2, bad, w1, e1)
        with pytest.raises(hl.ArgumentError, match="spartan: malformed instance"):
            hl.spartan_prove_relaxed(ctx, pp, key, bad, w1, e1)
    assert good()
    # a mask that wants fewer points than follow: the bytes left over read as two public inputs more
    fewer = b"\0" * 31 + b"\x01" + b1[32:]
    with pytest.raises(hl.ArgumentError, match="different numbers of public inputs"):
        fold(fewer, w1, e1, b2, w2, e2)
    with pytest.raises(hl.ArgumentError):
        hl.spartan_prove_relaxed(ctx, pp, key, fewer, w1, e1)
    assert good()
    with pytest.raises(hl.ArgumentError, match="different numbers of public inputs"):
        fold(b1, w1, e1, b2 + b"\0" * 32, w2, e2)
    with pytest.raises(hl.ArgumentError, match="num_public"):  # five public inputs in a half of four
        fold(b1 + b"\0" * 96, w1, e1, b2 + b"\0" * 96, w2, e2)
    # vectors of another size; a missing E for an instance whose C_E is a point
    with pytest.raises(hl.ArgumentError, match="a witness of"):
        fold(b1, hl.MultilinearPolynomial.new(ctx, [1] * (1 << l)), e1, b2, w2, e2)
    with pytest.raises(hl.ArgumentError, match="an error vector of"):
        fold(b1, w1, w1, b2, w2, e2)
    with pytest.raises(hl.ArgumentError, match="d_e"):
        hl.spartan_prove_relaxed(ctx, pp, key, b1, w1, None)
    assert good()
    # seven variables against the SRS of six is refused at the key already; through ctypes: the library's own answers on NULLs
    arr = lambda b: (C.c_uint8 * len(b)).from_buffer_copy(b)
    fr = lambda v: C.cast(C.c_void_p(v.ptr), C.POINTER(hl.lh_fr)) if v is not None else None
    a1, a2 = arr(b1), arr(b2)
    w_out, e_out = outs()
    out, room = (C.c_uint8 * 512)(), C.c_size_t(512)
    t = hl.Keccak256Transcript()
    args = lambda **o: [o.get(k, v) for k, v in (("ctx", ctx.h), ("pp", pp.h), ("key", key.h), ("a1", a1), ("n1", len(b1)), ("a2", a2),
                                                  ("n2", len(b2)), ("w1", fr(w1)), ("e1", fr(e1)), ("w2", fr(w2)), ("e2", None),
                                                  ("w_out", fr(w_out)), ("e_out", fr(e_out)), ("out", out), ("room", C.byref(room)),
                                                  ("t", t.p))]
    for hole in ("pp", "key", "a1", "a2", "w1", "w2", "w_out", "e_out", "out", "room", "t"):
        assert lib.lh_nova_fold(*args(**{hole: None})) == _ffi.LH_ERR_ARG, hole
    short = C.c_size_t(nv_bytes(p) - 1)
    assert lib.lh_nova_fold(*args(room=C.byref(short))) == _ffi.LH_ERR_ARG and b"LH_NOVA_INSTANCE_BYTES" in lib.lh_last_error()
    assert not t.into_proof(), "refused before a byte is written"
    room = C.c_size_t(nv_bytes(p))  # exactly LH_NOVA_INSTANCE_BYTES(p), with a first input that is itself that long
    assert len(b1) == nv_bytes(p)
    assert lib.lh_nova_fold(*args()) == _ffi.LH_OK and bytes(out[:room.value]) == slots[5][0] and t.into_proof() == records[5]["proof"]
    xs = hl._fr_array(nv.case_instance(case)[1][0][1])
    d_w = slots[0][1]
    room = C.c_size_t(512)
    assert lib.lh_nova_instance(ctx.h, None, key.h, fr(d_w), xs, p, out, C.byref(room)) == _ffi.LH_ERR_ARG
    assert lib.lh_nova_instance(ctx.h, pp.h, None, fr(d_w), xs, p, out, C.byref(room)) == _ffi.LH_ERR_ARG
    assert lib.lh_nova_instance(ctx.h, pp.h, key.h, None, xs, p, out, C.byref(room)) == _ffi.LH_ERR_ARG
    assert lib.lh_nova_instance(ctx.h, pp.h, key.h, fr(d_w), None, p, out, C.byref(room)) == _ffi.LH_ERR_ARG
    assert lib.lh_nova_instance(ctx.h, pp.h, key.h, fr(d_w), xs, p, None, C.byref(room)) == _ffi.LH_ERR_ARG
    assert lib.lh_nova_instance(ctx.h, pp.h, key.h, fr(d_w), xs, 0, out, C.byref(room)) == _ffi.LH_ERR_ARG
    assert lib.lh_nova_instance(ctx.h, pp.h, key.h, fr(d_w), xs, 5, out, C.byref(room)) == _ffi.LH_ERR_ARG
    assert lib.lh_nova_instance(ctx.h, pp.h, key.h, fr(d_w), xs, p, out, C.byref(room)) == _ffi.LH_OK and bytes(out[:room.value]) == slots[0][0]
    tp = hl.Keccak256Transcript()
    assert lib.lh_spartan_prove_relaxed(ctx.h, None, key.h, a1, len(b1), fr(w1), fr(e1), tp.p) == _ffi.LH_ERR_ARG
    assert lib.lh_spartan_prove_relaxed(ctx.h, pp.h, None, a1, len(b1), fr(w1), fr(e1), tp.p) == _ffi.LH_ERR_ARG
    assert lib.lh_spartan_prove_relaxed(ctx.h, pp.h, key.h, None, len(b1), fr(w1), fr(e1), tp.p) == _ffi.LH_ERR_ARG
    assert lib.lh_spartan_prove_relaxed(ctx.h, pp.h, key.h, a1, len(b1), None, fr(e1), tp.p) == _ffi.LH_ERR_ARG
    assert lib.lh_spartan_prove_relaxed(ctx.h, pp.h, key.h, a1, len(b1), fr(w1), fr(e1), None) == _ffi.LH_ERR_ARG
    assert not tp.into_proof()
    assert good()
    # a freed key is no longer one of the ctx's: refused without being read
    h = key.h
    key.free()
    room = C.c_size_t(512)
    assert lib.lh_nova_fold(*args(key=h)) == _ffi.LH_ERR_ARG and b"freed" in lib.lh_last_error()
    assert lib.lh_nova_instance(ctx.h, pp.h, h, fr(d_w), xs, p, out, C.byref(room)) == _ffi.LH_ERR_ARG and b"freed" in lib.lh_last_error()
    assert lib.lh_spartan_prove_relaxed(ctx.h, pp.h, h, a1, len(b1), fr(w1), fr(e1), tp.p) == _ffi.LH_ERR_ARG and b"freed" in lib.lh_last_error()
    with pytest.raises(hl.ArgumentError, match="freed"):
        fold(b1, w1, e1, b2, w2, e2)
    assert good()


def nv_bytes(p):
    return 160 + 32 * p


# ------------------------------------------------------------------ 5. the plain prover after folds on the same ctx and key
def test_the_plain_prover_is_unmoved_after_folds(hl, ctx, kzg6):
    pp, vp = kzg6
    case = "square"
    n, l, p = spa.CASES[case]
    inst, assigns = spa.case_instance(case)
    w, x = assigns[0]
    rec = SPARTAN_GOLDEN[case]["proofs"][0]
    with _commit(hl, ctx, pp, inst, l) as key:
        d_w = hl.MultilinearPolynomial.new(ctx, w)
        # square's own assignment, fresh, folded with itself and proved relaxed - then the plain proof of the same key
        blob = hl.nova_instance(ctx, pp, key, d_w, x)
        w_out, e_out = _vector(hl, ctx, l - 1), _vector(hl, ctx, l)
        folded, proof = hl.nova_fold(ctx, pp, key, blob, d_w, None, blob, d_w, None, w_out, e_out)
        assert len(proof) == 32 and hl.nova_fold_verify(n, l, key.commitment, blob, blob, proof) == folded
        hl.spartan_verify_relaxed(vp, n, l, key.commitment, folded, p, hl.spartan_prove_relaxed(ctx, pp, key, folded, w_out, e_out))
        plain = hl.spartan_prove(ctx, pp, key, d_w, x)
        assert (len(plain), hashlib.sha256(plain).hexdigest()) == (rec["bytes"], rec["sha256"])
        hl.spartan_verify(vp, n, l, key.commitment, x, plain)
