"""Regenerate tests/golden/spartan_batch.json: batched Spartan proofs over multilinear KZG from the Python oracle extended by
tests/spark_ref.py, tests/spartan_ref.py and tests/spartan_batch_ref.py (the other generators and fixtures stay as they are).

    python tests/golden/make_spartan_batch.py

The SRS secrets of the cases up to six variables are tests/golden/lasso_tables.json's; `mid` uses the seeded 14 secrets of
logup_gkr_ref.mid_ss().  Records, for every case of spartan_batch_ref.CASES, its shape, length and SHA-256 of its key blob,
the public inputs instance by instance, the proof's length and its SHA-256 (`twice`, which the PCS refuses - see
spartan_batch_ref.REFUSED -: the words and the bytes written before them) (instances and witnesses follow from the case's
seeds, and for the six-variable cases so do key and proof bytes: whoever needs them runs the specification and compares the
digest; `mid` is recorded in full); for every forgery of spartan_batch_ref.FORGERIES the public inputs the verifier is
given, length and digest.
Before the file is written the dense relation holds for every instance of every six-variable case (`mid`: the sparse count,
per instance, by spartan_ref's own keyed sum), the specification's verifier accepts every honest proof and refuses every
forgery with its words.
"""
import hashlib
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import logup_gkr_ref as lgr  # noqa: E402
import spartan_batch_ref as sbr  # noqa: E402
import spartan_ref as spa  # noqa: E402
from oracle.pyref import kzg  # noqa: E402
from oracle.pyref.field import R_MOD as P  # noqa: E402
from oracle.pyref.transcript import Keccak256Transcript as T  # noqa: E402
from oracle.pyref.transcript import TranscriptError  # noqa: E402


def pinned(xs, proof, full):
    rec = {"xs": [["%x" % v for v in x] for x in xs], "bytes": len(proof), "sha256": hashlib.sha256(proof).hexdigest()}
    if full:
        rec["proof"] = proof.hex()
    return rec


def pinned_key(blob, full):
    rec = {"key_bytes": len(blob), "key_sha256": hashlib.sha256(blob).hexdigest()}
    if full:
        rec["key"] = blob.hex()
    return rec


def honest(pp, case):
    n, l, p, count = sbr.CASES[case]
    full = case not in sbr.SMALL
    inst, ws, xs = sbr.case_instance(case)
    key = spa.commit(pp, inst, l)
    if l <= 6:
        assert sbr.satisfied(inst, ws, xs, l) == (0, None), case
    else:  # (the dense statement of `mid` is 2^20 cells a matrix)
        for w, x in zip(ws, xs):
            z = spa.assignment(l, w, x)
            a, b, c = [spa.spmv(m.dims[0], m.dims[1], m.val, z, 1 << l) for m in key.mats]
            assert all((u * v - t) % P == 0 for u, v, t in zip(a, b, c)), case
    t = T()
    if case in sbr.REFUSED:  # (the opening's transcript refuses: the words and what was written before them)
        try:
            sbr.prove(pp, key, ws, xs, t)
        except TranscriptError as e:
            assert re.search(sbr.REFUSED[case], str(e)), (case, str(e))
        else:
            raise AssertionError("the case %s was proved" % case)
        written = t.into_proof()
        return dict({"n": n, "l": l, "p": p, "count": count, "error": sbr.REFUSED[case]}, **pinned_key(key.blob, full),
                    **pinned(xs, written, full))
    sbr.prove(pp, key, ws, xs, t)
    proof = t.into_proof()
    sbr.verify(pp, n, l, key.blob, xs, T(proof))
    return dict({"n": n, "l": l, "p": p, "count": count}, **pinned_key(key.blob, full), **pinned(xs, proof, full))


def forged(pp, name):
    case, ws, xs, xs_verified, forge = sbr.forgery(name)
    n, l, p, _ = sbr.CASES[case]
    inst, _, _ = sbr.case_instance(case)
    key = spa.commit(pp, inst, l)
    t = T()
    sbr.prove(pp, key, ws, xs, t, forge=forge)
    proof = t.into_proof()
    try:
        sbr.verify(pp, n, l, key.blob, xs_verified, T(proof))
    except spa.SpartanError as e:
        assert re.search(sbr.FORGERIES[name], str(e)), (name, str(e))
    else:
        raise AssertionError("the forged proof %s verified" % name)
    return dict(pinned(xs_verified, proof, full=False), case=case)


def main():
    ss = [int(x, 16) for x in json.load(open(os.path.join(HERE, "lasso_tables.json")))["srs"]["ss"]]
    pps = {False: kzg.setup(ss), True: None}
    out = {"mid_srs_seed": lgr.MID_SRS_SEED, "cases": {}, "forgeries": {}}
    for case in sbr.CASES:
        big = case not in sbr.SMALL
        if big and pps[True] is None:
            pps[True] = kzg.setup(lgr.mid_ss())
        out["cases"][case] = honest(pps[big], case)
    for name in sbr.FORGERIES:
        out["forgeries"][name] = forged(pps[False], name)
    with open(os.path.join(HERE, "spartan_batch.json"), "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()
