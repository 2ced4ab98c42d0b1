"""Regenerate tests/golden/lasso_tables.json: Lasso proofs over multilinear KZG into the OR / EQ / LTU subtables, from the
Python oracle extended by tests/lasso_tables_ref.py (make_golden.py and vectors.json stay as they are).

    python tests/golden/make_golden_lasso_tables.py

Records the SRS secrets, the chunk columns and the proof of: or (2,4,5), equal (4,2,3), less_than (4,4,6), less_than (1,2,1)
- (c, l, n) each.  The oracle's own verifier accepts every proof before it is written.
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lasso_tables_ref as ltr  # noqa: E402
from oracle.pyref import kzg, lasso  # noqa: E402
from oracle.pyref.field import R_MOD as P  # noqa: E402
from oracle.pyref.transcript import Keccak256Transcript as T  # noqa: E402

CASES = (("or", 2, 4, 5), ("equal", 4, 2, 3), ("less_than", 4, 4, 6), ("less_than", 1, 2, 1))


def main():
    rng = random.Random(20231216)
    ss = [rng.randrange(1, P) for _ in range(6)]
    pp = kzg.setup(ss)
    out = {"srs": {"ss": ["%x" % s for s in ss]}, "lasso": []}
    with ltr.installed():
        for kind, c, l, n in CASES:
            spec = ltr.spec_of(kind, c, l)
            dims = [[rng.randrange(1 << l) for _ in range(1 << n)] for _ in range(c)]
            if kind == "equal":  # (random 4-bit operands are rarely equal: make half of the lookups hits)
                for k in range(0, 1 << n, 2):
                    for j in range(c):
                        dims[j][k] = (dims[j][k] >> (l // 2)) * ((1 << (l // 2)) + 1)
            t = T()
            lasso.prove(pp, spec, dims, t)
            proof = t.into_proof()
            lasso.verify(pp, spec, n, T(proof))
            out["lasso"].append({"kind": kind, "c": c, "l": l, "n": n, "dims": dims, "proof": proof.hex()})
    with open(os.path.join(HERE, "lasso_tables.json"), "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()
