"""Writes tests/golden/ligero.json: for each case of tests/ligero_ref.py GOLDEN_CASES the parameters, the root, the evaluation,
and the length and SHA-256 digest of the specification's opening proof; the proof of the case GOLDEN_FULL is stored whole
beside it, as raw bytes in tests/golden/ligero_<case>.proof (219 KiB).  The other proofs are made again from their seeds by the tests and checked against these digests.  A few seconds.

    python tests/golden/make_ligero.py
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import ligero_ref as lr  # noqa: E402


def main():
    out = {}
    for case in lr.GOLDEN_CASES:
        pp, root, point, value, proof = lr.golden_proof(case)
        rec = {"case": list(case), "info": list(pp.info()), "depth": pp.depth, "root": root.hex(), "value": "%064x" % value,
               "proof_len": len(proof), "proof_sha256": hashlib.sha256(proof).hexdigest()}
        if case == lr.GOLDEN_FULL:
            rec["point"] = ["%064x" % x for x in point]
            rec["proof_file"] = "ligero_%s.proof" % lr.golden_name(case)
            with open(os.path.join(HERE, rec["proof_file"]), "wb") as f:
                f.write(proof)
        out[lr.golden_name(case)] = rec
        print(lr.golden_name(case), rec["info"], len(proof), flush=True)
    with open(os.path.join(HERE, "ligero.json"), "w") as f:
        f.write("{\n" + ",\n".join(json.dumps(k) + ": " + json.dumps(out[k], sort_keys=True) for k in sorted(out)) + "\n}\n")


if __name__ == "__main__":
    main()
