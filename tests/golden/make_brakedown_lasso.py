"""Writes tests/golden/brakedown_lasso.json: for each case of tests/brakedown_lasso_ref.py the parameters' shape, the number
of evaluations, the length and SHA-256 digest of the oracle's Lasso-over-Brakedown proof, and the roots it wrote.  The proofs
themselves (4-20 MB) are not stored.  Takes a minute or two.

    python tests/golden/make_brakedown_lasso.py
"""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import brakedown_lasso_ref as bl  # noqa: E402


def main():
    out = {}
    for name in bl.CASES:
        t = time.time()
        out[name] = bl.record(name)
        print("case %s %r: %d bytes, %d evaluations, %.1f s" % (name, bl.CASES[name][:4], out[name]["proof_len"],
                                                               out[name]["num_evaluations"], time.time() - t), flush=True)
    with open(bl.FIXTURE, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
