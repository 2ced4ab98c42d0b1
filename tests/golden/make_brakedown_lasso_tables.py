"""Writes tests/golden/brakedown_lasso_tables.json: Lasso over MultilinearBrakedown into the EQ / LTU subtables - the oracle's
prover (oracle/pyref/lasso.py under the wrappers of tests/lasso_tables_ref.py) over the Brakedown adapter of
tests/brakedown_provers_ref.py, as tests/brakedown_lasso_ref.py runs it for the old tables.  Per case the parameters' shape,
the length and SHA-256 digest of the proof and the roots it wrote, in order; the proofs themselves (megabytes) are not stored.

    python tests/golden/make_brakedown_lasso_tables.py
"""
import hashlib
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import brakedown_lasso_ref as bl  # noqa: E402
import brakedown_provers_ref as bp  # noqa: E402
import brakedown_ref as br  # noqa: E402
import lasso_tables_ref as ltr  # noqa: E402
from oracle.pyref import lasso as o_lasso  # noqa: E402

CASES = (("less_than", 2, 4, 5), ("equal", 2, 4, 5))
FIXTURE = os.path.join(HERE, "brakedown_lasso_tables.json")


def record(kind, c, l, n):
    spec, dims, nv = ltr.spec_of(kind, c, l), ltr.random_dims(kind, c, l, n), max(n, l)
    pp = br.Params(nv, bl.SPEC, bl.SEED)
    written = []

    class Recording(bl.Transcript):
        def write_commitments(self, comms):
            written.extend(cm.root for cm in comms)
            super().write_commitments(comms)
    tr = Recording()
    with ltr.installed():
        o_lasso.prove(pp, spec, dims, tr, bp.BrakedownPcs())
    proof = tr.into_proof()
    assert len(written) == 1 + 3 * spec.c + spec.alpha
    return {"case": [kind, c, l, n], "num_vars": nv, "spec": bl.SPEC, "num_rows": pp.num_rows, "row_len": pp.row_len,
            "codeword_len": pp.codeword_len, "proof_len": len(proof), "proof_sha256": hashlib.sha256(proof).hexdigest(),
            "roots": [r.hex() for r in written]}


def main():
    out = {}
    for case in CASES:
        t = time.time()
        out["%s-%d-%d-%d" % case] = record(*case)
        print("%r: %d bytes, %.1f s" % (case, out["%s-%d-%d-%d" % case]["proof_len"], time.time() - t), flush=True)
    with open(FIXTURE, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
