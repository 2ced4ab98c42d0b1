"""Regenerate tests/golden/nova.json: Nova folds and relaxed Spartan proofs over multilinear KZG from the Python oracle
extended by tests/spark_ref.py, tests/spartan_ref.py and tests/nova_ref.py (the other generators and fixtures stay as they are).

    python tests/golden/make_nova.py

The SRS secrets of the cases up to six variables are tests/golden/lasso_tables.json's; `mid` uses the seeded 14 secrets of
logup_gkr_ref.mid_ss().  Records, for every case of nova_ref.CASES, its shape, length and SHA-256 of its key blob and per step
of its schedule (nova_ref.SCHEDULES) length and SHA-256 of what the step makes: a fresh instance's blob, a fold's proof and
folded blob, the relaxed proof (instances and witnesses follow from the case's seeds, and for the six-variable cases so do
all bytes: whoever needs them runs the specification and compares the digest; `mid` is recorded in full); for every forgery of
nova_ref.FORGERIES the blob the relaxed verifier is given and the proof, by length and digest.
Before the file is written the dense relaxed relation holds for every fresh and every folded pair (six-variable cases),
every folded commitment equals a direct commitment of the folded vector, the fold verifier returns the prover's blob, the
relaxed verifier accepts every honest proof and refuses every forgery with its words.
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
import nova_ref as nv  # noqa: E402
import spartan_ref as spa  # noqa: E402
from oracle.pyref import kzg  # noqa: E402
from oracle.pyref.transcript import Keccak256Transcript as T  # noqa: E402


def pin(prefix, data, full):
    rec = {prefix + "bytes": len(data), prefix + "sha256": hashlib.sha256(data).hexdigest()}
    if full:
        rec[prefix.rstrip("_") or "data"] = data.hex()
    return rec


def check_slots(pp, key, case, slots, records):
    """the three things that hold before a byte is recorded"""
    n, l, p = nv.CASES[case]
    inst, _ = nv.case_instance(case)
    for (U, (w, E)), rec in zip(slots, [r for r in records if r["step"] != "prove"]):
        if l <= 6:
            assert nv.relaxed_satisfied(inst, w, E, U.x, l) == 0, (case, "the dense relaxed relation")
        else:
            assert nv.unsatisfied(nv.products(key, w, U.x), U.x[0], E) == 0, case
        assert U.cw == kzg.commit(pp.trim(l - 1), w), (case, "C_W is the commitment of the folded w")
        assert U.ce == (kzg.commit(pp.trim(l), E) if E is not None else None), (case, "C_E is the commitment of the folded E")
        assert nv.read_instance(U.blob, p).blob == U.blob == rec["blob"]


def honest(pp, case):
    n, l, p = nv.CASES[case]
    full = case not in nv.SMALL
    inst, _ = nv.case_instance(case)
    key = spa.commit(pp, inst, l)
    slots, records = nv.run(pp, key, case)
    check_slots(pp, key, case, slots, records)
    blobs = [r["blob"] for r in records if r["step"] != "prove"]
    steps = []
    for r in records:
        if r["step"] == "fresh":
            steps.append(dict({"step": "fresh"}, **pin("blob_", r["blob"], full)))
        elif r["step"] == "fold":
            assert len(r["proof"]) == (32 if case == "self_fold" else 96), (case, "a cross term is zero in self_fold alone")
            assert nv.fold_verify(n, l, p, key.blob, blobs[r["a"]], blobs[r["b"]], T(r["proof"])) == r["blob"], case
            steps.append(dict({"step": "fold", "a": r["a"], "b": r["b"]}, **pin("proof_", r["proof"], full), **pin("blob_", r["blob"], full)))
        else:
            nv.verify_relaxed(pp, n, l, p, key.blob, blobs[r["a"]], T(r["proof"]))
            steps.append(dict({"step": "prove", "a": r["a"]}, **pin("proof_", r["proof"], full)))
    return dict({"n": n, "l": l, "p": p}, **pin("key_", key.blob, full), steps=steps)


def forgery(pp, name):
    """-> (key blob, the instance blob the relaxed verifier is given, the proof)"""
    case = nv.FORGERY_CASE
    n, l, p = nv.CASES[case]
    inst, _ = nv.case_instance(case)
    key = spa.commit(pp, inst, l)
    slots, records = nv.run(pp, key, case, forge=name if name != "other_input" else None)
    blobs = [r["blob"] for r in records if r["step"] != "prove"]
    last = [r for r in records if r["step"] == "fold"][-1]
    proof = records[-1]["proof"]
    if name == "bad_T":  # the fold verifies: nothing in it is checked
        blob = nv.fold_verify(n, l, p, key.blob, blobs[last["a"]], blobs[last["b"]], T(last["proof"]))
        assert blob == last["blob"]
    elif name == "bad_vE":
        blob = last["blob"]
    else:  # the last fold's proof against another second input
        blob = nv.fold_verify(n, l, p, key.blob, blobs[last["a"]], blobs[1], T(last["proof"]))
        assert blob != last["blob"] and last["b"] != 1
    return key.blob, blob, proof


def forged(pp, name):
    case = nv.FORGERY_CASE
    n, l, p = nv.CASES[case]
    key_blob, blob, proof = forgery(pp, name)
    try:
        nv.verify_relaxed(pp, n, l, p, key_blob, blob, T(proof))
    except spa.SpartanError as e:
        assert re.search(nv.FORGERIES[name], str(e)), (name, str(e))
    else:
        raise AssertionError("the forged proof %s verified" % name)
    return dict({"case": case}, **pin("blob_", blob, False), **pin("proof_", proof, False))


def main():
    ss = [int(x, 16) for x in json.load(open(os.path.join(HERE, "lasso_tables.json")))["srs"]["ss"]]
    pps = {False: kzg.setup(ss), True: None}
    out = {"mid_srs_seed": lgr.MID_SRS_SEED, "cases": {}, "forgeries": {}}
    for case in nv.CASES:
        big = case not in nv.SMALL
        if big and pps[True] is None:
            pps[True] = kzg.setup(lgr.mid_ss())
        out["cases"][case] = honest(pps[big], case)
    for name in nv.FORGERIES:
        out["forgeries"][name] = forged(pps[False], name)
    with open(os.path.join(HERE, "nova.json"), "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()
