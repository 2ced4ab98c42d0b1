"""Regenerate tests/golden/spartan.json: Spartan keys and proofs over multilinear KZG from the Python oracle extended by
tests/spark_ref.py and tests/spartan_ref.py (the other generators and fixtures stay as they are).

    python tests/golden/make_spartan.py

The SRS secrets of the cases up to six variables are tests/golden/lasso_tables.json's; `mid` uses the seeded 14 secrets of
logup_gkr_ref.mid_ss().  Records, for every case of spartan_ref.CASES, its shape, length and SHA-256 of its key blob and per
assignment the public input, the proof's length and its SHA-256 (instance and witness follow from the case's seeds, and for
the six-variable cases so do key and proof bytes: whoever needs them runs the specification and compares the digest; `mid`,
which takes half a minute, is recorded in full); for every forgery of spartan_ref.FORGERIES the public input the verifier is given, length and digest.
Before the file is written `satisfied` (dense matrices) holds for every
honest assignment, the specification's verifier accepts every honest proof and refuses every forgery with its words.
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
import spartan_ref as spa  # noqa: E402
from oracle.pyref import kzg  # noqa: E402
from oracle.pyref.transcript import Keccak256Transcript as T  # noqa: E402


def pinned(x, proof, full):
    rec = {"x": ["%x" % v for v in x], "bytes": len(proof), "sha256": hashlib.sha256(proof).hexdigest()}
    if full:
        rec["proof"] = proof.hex()
    return rec


def pinned_key(blob, full):
    rec = {"key_bytes": len(blob), "key_sha256": hashlib.sha256(blob).hexdigest()}
    if full:
        rec["key"] = blob.hex()
    return rec


def honest(pp, case):
    n, l, p = spa.CASES[case]
    inst, assigns = spa.case_instance(case)
    key = spa.commit(pp, inst, l)
    proofs = []
    for w, x in assigns:
        if l <= 6:  # (the dense statement of `mid` is 2^20 cells a matrix: the sparse count inside prove stands for it)
            assert spa.satisfied(inst, w, x, l) == 0, case
        t = T()
        spa.prove(pp, key, w, x, t)
        proof = t.into_proof()
        spa.verify(pp, n, l, key.blob, x, T(proof))
        proofs.append(pinned(x, proof, full=case not in spa.SMALL))
    return dict({"n": n, "l": l, "p": p}, **pinned_key(key.blob, full=case not in spa.SMALL), proofs=proofs)


def forged(pp, name):
    case, w, x, x_verified, forge = spa.forgery(name)
    n, l, p = spa.CASES[case]
    inst, _ = spa.case_instance(case)
    key = spa.commit(pp, inst, l)
    t = T()
    spa.prove(pp, key, w, x, t, forge=forge)
    proof = t.into_proof()
    try:
        spa.verify(pp, n, l, key.blob, x_verified, T(proof))
    except spa.SpartanError as e:
        assert re.search(spa.FORGERIES[name], str(e)), (name, str(e))
    else:
        raise AssertionError("the forged proof %s verified" % name)
    return dict(pinned(x_verified, proof, full=False), case=case)


def main():
    ss = [int(x, 16) for x in json.load(open(os.path.join(HERE, "lasso_tables.json")))["srs"]["ss"]]
    pps = {False: kzg.setup(ss), True: None}
    out = {"mid_srs_seed": lgr.MID_SRS_SEED, "cases": {}, "forgeries": {}}
    for case in spa.CASES:
        big = case not in spa.SMALL
        if big and pps[True] is None:
            pps[True] = kzg.setup(lgr.mid_ss())
        out["cases"][case] = honest(pps[big], case)
    for name in spa.FORGERIES:
        out["forgeries"][name] = forged(pps[False], name)
    with open(os.path.join(HERE, "spartan.json"), "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()
