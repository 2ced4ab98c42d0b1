"""Regenerate tests/golden/memcheck.json: read-write memory-checking proofs over multilinear KZG from the Python oracle
extended by tests/memcheck_ref.py (the other generators and fixtures stay as they are).

    python tests/golden/make_memcheck.py

The SRS secrets of the cases up to six variables are tests/golden/lasso_tables.json's; `mid` uses the seeded 14 secrets of
logup_gkr_ref.mid_ss().  Records, for every case of memcheck_ref.CASES, its shape and its proof (trace and image follow
from the case's seeds), and for the two cheating provers of memcheck_ref.forgery their traces and proofs.  The
specification's own verifier accepts every honest proof, and refuses every forged one where it should, before the file is
written.  `mid` takes about a minute.
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import logup_gkr_ref as lgr  # noqa: E402
import memcheck_ref as mcr  # noqa: E402
from oracle.pyref import kzg  # noqa: E402
from oracle.pyref.transcript import Keccak256Transcript as T  # noqa: E402


def honest(pp, case):
    n, l, has_init = mcr.CASES[case]
    init = mcr.case_init(case)
    t = T()
    mcr.prove(pp, *mcr.case_trace(case), l, init, t)
    proof = t.into_proof()
    mcr.verify(pp, n, l, init, T(proof))
    return {"n": n, "l": l, "init": has_init, "proof": proof.hex()}


def forged(pp, name):
    n, l, trace, forge = mcr.forgery(name)
    t = T()
    mcr.prove(pp, *trace, l, None, t, forge=forge)
    proof = t.into_proof()
    try:
        mcr.verify(pp, n, l, None, T(proof))
    except mcr.MemcheckError as e:
        assert re.search(mcr.FORGERIES[name], str(e)), (name, str(e))
    else:
        raise AssertionError("the forged proof %s verified" % name)
    return {"n": n, "l": l, "addr": trace[0], "rv": trace[1], "wv": trace[2], "proof": proof.hex()}


def main():
    ss = [int(x, 16) for x in json.load(open(os.path.join(HERE, "lasso_tables.json")))["srs"]["ss"]]
    pps = {False: kzg.setup(ss), True: None}
    out = {"mid_srs_seed": lgr.MID_SRS_SEED, "cases": {}, "forgeries": {}}
    for case in mcr.CASES:
        big = case not in mcr.SMALL
        if big and pps[True] is None:
            pps[True] = kzg.setup(lgr.mid_ss())
        out["cases"][case] = honest(pps[big], case)
    for name in mcr.FORGERIES:
        out["forgeries"][name] = forged(pps[False], name)
    with open(os.path.join(HERE, "memcheck.json"), "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()
