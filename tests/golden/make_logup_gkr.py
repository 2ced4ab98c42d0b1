"""Regenerate tests/golden/logup_gkr.json: LogUp-GKR proofs over multilinear KZG from the Python oracle extended by
tests/logup_gkr_ref.py (the other generators and fixtures stay as they are).

    python tests/golden/make_logup_gkr.py

The SRS secrets of the cases up to six variables are tests/golden/lasso_tables.json's; `mid` uses the seeded 14 secrets of
logup_gkr_ref.mid_ss().  Records, for every case of logup_gkr_ref.CASES, its shape, the table row of every input row and
the proof (tables and inputs follow from the case's seeds).  The specification's own verifier accepts every proof before
it is written.  `mid` takes about half a minute.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import logup_gkr_ref as lgr  # noqa: E402
from oracle.pyref import kzg  # noqa: E402
from oracle.pyref.transcript import Keccak256Transcript as T  # noqa: E402


def main():
    ss = [int(x, 16) for x in json.load(open(os.path.join(HERE, "lasso_tables.json")))["srs"]["ss"]]
    pps = {False: kzg.setup(ss), True: None}
    out = {"mid_srs_seed": lgr.MID_SRS_SEED, "cases": {}}
    for case, (n, l, widths) in lgr.CASES.items():
        big = case not in lgr.SMALL
        if big and pps[True] is None:
            pps[True] = kzg.setup(lgr.mid_ss())
        pp = pps[big]
        lookups = lgr.case_lookups(case)
        t = T()
        lgr.prove(pp, lookups, t)
        proof = t.into_proof()
        lgr.verify(pp, [tb for _, tb in lookups], n, T(proof))
        out["cases"][case] = {"n": n, "l": l, "widths": widths, "rows": lgr.case_rows(case), "proof": proof.hex()}
    with open(os.path.join(HERE, "logup_gkr.json"), "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()
