"""Regenerate tests/golden/spark.json: Spark commitments and opening proofs over multilinear KZG from the Python oracle
extended by tests/spark_ref.py (the other generators and fixtures stay as they are).

    python tests/golden/make_spark.py

The SRS secrets of the cases up to six variables are tests/golden/lasso_tables.json's; `mid` and `wide` use the seeded 14
secrets of logup_gkr_ref.mid_ss().  Records, for every case of spark_ref.CASES, its shape, its commitment, and per opening
the point, the value and the proof (the entries follow from the case's seeds); for the cheating prover of
spark_ref.forgery its entries, point, claimed value and proof; and `bad_value`, an honest proof with another value.  The
specification's own verifier accepts every honest proof and refuses every forged one where it should before the file is
written; every value equals the defining sum.  `mid` and `wide` take about a minute each.
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
import spark_ref as spr  # noqa: E402
from oracle.pyref import kzg  # noqa: E402
from oracle.pyref.field import R_MOD as P  # noqa: E402
from oracle.pyref.transcript import Keccak256Transcript as T  # noqa: E402


def honest(pp, case):
    n, l, c = spr.CASES[case]
    dims, val = spr.case_entries(case)
    cm = spr.commit(pp, dims, val, l)
    openings = []
    for point in spr.case_points(case):
        t = T()
        v = spr.open_(pp, cm, point, t)
        proof = t.into_proof()
        assert v == spr.sparse_eval(dims, val, l, point), case
        spr.verify(pp, n, l, c, cm.blob, point, v, T(proof))
        openings.append({"point": ["%x" % x for x in point], "value": "%x" % v, "proof": proof.hex()})
    return {"n": n, "l": l, "c": c, "commitment": cm.blob.hex(), "openings": openings}


def forged(pp, name):
    n, l, c, dims, val, point, forge = spr.forgery(name)
    cm = spr.commit(pp, dims, val, l)
    t = T()
    v = spr.open_(pp, cm, point, t, forge=forge)
    proof = t.into_proof()
    try:
        spr.verify(pp, n, l, c, cm.blob, point, v, T(proof))
    except spr.SparkError as e:
        assert re.search(spr.FORGERIES[name], str(e)), (name, str(e))
    else:
        raise AssertionError("the forged proof %s verified" % name)
    return {"n": n, "l": l, "c": c, "dims": dims, "val": val, "commitment": cm.blob.hex(), "point": ["%x" % x for x in point],
            "value": "%x" % v, "proof": proof.hex()}


def main():
    ss = [int(x, 16) for x in json.load(open(os.path.join(HERE, "lasso_tables.json")))["srs"]["ss"]]
    pps = {False: kzg.setup(ss), True: None}
    out = {"mid_srs_seed": lgr.MID_SRS_SEED, "cases": {}, "forgeries": {}}
    for case in spr.CASES:
        big = case not in spr.SMALL
        if big and pps[True] is None:
            pps[True] = kzg.setup(lgr.mid_ss())
        out["cases"][case] = honest(pps[big], case)
    for name in spr.FORGERIES:
        out["forgeries"][name] = forged(pps[False], name)
    # an honest proof against another value: refused where the value is read
    g = out["cases"]["matrix"]
    o = g["openings"][0]
    wrong = (int(o["value"], 16) + 1) % P
    try:
        spr.verify(pps[False], g["n"], g["l"], g["c"], bytes.fromhex(g["commitment"]), [int(x, 16) for x in o["point"]], wrong,
                   T(bytes.fromhex(o["proof"])))
    except spr.SparkError as e:
        assert "another value" in str(e)
    else:
        raise AssertionError("a wrong value verified")
    out["bad_value"] = {"case": "matrix", "value": "%x" % wrong}
    with open(os.path.join(HERE, "spark.json"), "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()
