"""Writes tests/golden/brakedown_hyperplonk.json: for each case of tests/brakedown_provers_ref.py the parameters' shape, the
number of evaluations, the length and SHA-256 digest of the oracle's HyperPlonk-over-Brakedown proof, and the preprocess and
permutation roots.  The proofs themselves (8 MB and up) are not stored.  Takes a few minutes.

    python tests/golden/make_brakedown_hyperplonk.py
"""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import brakedown_provers_ref as bp  # noqa: E402


def main():
    out = {}
    for name, case in bp.cases().items():
        t = time.time()
        out[name] = bp.record(case)
        print("case %s %r: %d bytes, %d evaluations, %.1f s" % (name, case, out[name]["proof_len"],
                                                               out[name]["num_evaluations"], time.time() - t), flush=True)
    with open(bp.FIXTURE, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
