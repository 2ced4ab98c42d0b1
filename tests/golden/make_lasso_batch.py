"""Regenerate tests/golden/lasso_batch.json: batch Lasso proofs (several tables, one proof) over multilinear KZG from the
Python oracle extended by tests/lasso_batch_ref.py (the other generators and fixtures stay as they are).

    python tests/golden/make_lasso_batch.py

The SRS secrets are tests/golden/lasso_tables.json's.  Records, for every case of lasso_batch_ref.CASES, the chunk columns of
every table and the proof; a case of lasso_batch_ref.SHARED records its columns once.  The reference's own verifier accepts
every proof before it is written.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lasso_batch_ref as lbr  # noqa: E402
import lasso_custom_ref as lcr  # noqa: E402
from oracle.pyref import kzg  # noqa: E402
from oracle.pyref.transcript import Keccak256Transcript as T  # noqa: E402


def main():
    ss = [int(x, 16) for x in json.load(open(os.path.join(HERE, "lasso_tables.json")))["srs"]["ss"]]
    pp = kzg.setup(ss)
    out = {"cases": {}}
    for case, (n, descs) in lbr.CASES.items():
        dims = lbr.case_dims(case)
        specs = [lbr.spec_of(d) for d in descs]
        with lcr.installed(lbr.custom_values(case)):
            t = T()
            lbr.prove(pp, specs, dims, t)
            proof = t.into_proof()
            lbr.verify(pp, specs, n, T(proof))
        out["cases"][case] = {"n": n, "dims": dims[:1] if case in lbr.SHARED else dims, "proof": proof.hex()}
    with open(os.path.join(HERE, "lasso_batch.json"), "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()
