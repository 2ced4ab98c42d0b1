"""Regenerate tests/golden/lasso_custom.json: Lasso proofs over multilinear KZG into caller-registered subtables, from the
Python oracle extended by tests/lasso_custom_ref.py (the other generators and fixtures stay as they are).

    python tests/golden/make_lasso_custom.py

The SRS secrets are tests/golden/lasso_tables.json's.  Records the named table, the shape, the chunk columns and the proof of
every case of lasso_custom_ref.CASES and of less_than_signed(2, 4) at n = 5.  A custom kind is not absorbed into the
transcript: the fixed numbers used here stand for whatever kinds a registry hands out.  The oracle's own verifier accepts
every proof before it is written.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lasso_custom_ref as lcr  # noqa: E402
from oracle.pyref import kzg, lasso  # noqa: E402
from oracle.pyref.transcript import Keccak256Transcript as T  # noqa: E402

KIND = lcr.CUSTOM_BASE + 7  # (any custom kind)


def main():
    ss = [int(x, 16) for x in json.load(open(os.path.join(HERE, "lasso_tables.json")))["srs"]["ss"]]
    pp = kzg.setup(ss)
    out = {"lasso": []}

    def record(entry, spec, values, dims, n):
        with lcr.installed({KIND: values}):
            t = T()
            lasso.prove(pp, spec, dims, t)
            proof = t.into_proof()
            lasso.verify(pp, spec, n, T(proof))
        entry.update({"n": n, "dims": dims, "proof": proof.hex()})
        out["lasso"].append(entry)

    for name, c, n, g in lcr.CASES:
        l = lcr.bits_of(lcr.TABLES[name])
        record({"table": name, "c": c, "l": l, "g": g}, lcr.spec_of(name, c, g, KIND), lcr.TABLES[name],
               lcr.random_dims(name, c, l, n), n)
    c, l, n = 2, 4, 5
    record({"table": "less_than_signed", "c": c, "l": l, "g": "less_than_signed"}, lcr.less_than_signed_spec(c, l, KIND),
           lcr.lts_values(l), lcr.comparison_dims(c, l, n), n)
    with open(os.path.join(HERE, "lasso_custom.json"), "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()
