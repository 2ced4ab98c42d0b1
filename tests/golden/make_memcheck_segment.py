"""Regenerate tests/golden/memcheck_segment.json: segment proofs of the read-write memory-checking argument - the image a
committed column - over multilinear KZG, from the Python oracle extended by tests/memcheck_segment_ref.py (the other
generators and fixtures stay as they are).

    python tests/golden/make_memcheck_segment.py

The SRS secrets of the cases up to six variables are tests/golden/lasso_tables.json's; `mid` uses the seeded 14 secrets of
logup_gkr_ref.mid_ss().  Records, for every case of memcheck_segment_ref.CASES, its shape, its proof and the two
commitments the verifier returns (image, final values; null: the identity), the chain of three segments, and for the
three cheating provers their images, traces and proofs.  The specification's own verifier accepts every honest proof, and
refuses every forged one where it should, before the file is written.  `mid` takes about a minute.
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
import memcheck_segment_ref as msr  # noqa: E402
from oracle.pyref import kzg  # noqa: E402
from oracle.pyref.transcript import Keccak256Transcript as T  # noqa: E402


def point(pt):
    return None if pt is None else ["%x" % pt[0], "%x" % pt[1]]


def segment(pp, n, l, trace, image):
    t = T()
    fv = msr.prove(pp, *trace, l, image, t)
    proof = t.into_proof()
    iv_c, fv_c = msr.verify(pp, n, l, T(proof))
    return {"n": n, "l": l, "proof": proof.hex(), "image_commitment": point(iv_c), "final_commitment": point(fv_c)}, fv


def forged(pp, name):
    n, l, image, trace, forge = msr.forgery(name)
    t = T()
    msr.prove(pp, *trace, l, image, t, forge=forge)
    proof = t.into_proof()
    try:
        msr.verify(pp, n, l, T(proof))
    except (msr.MemcheckError, kzg.PcsError) as e:
        assert re.search(msr.FORGERIES[name], str(e)), (name, str(e))
    else:
        raise AssertionError("the forged proof %s verified" % name)
    return {"n": n, "l": l, "image": image, "addr": trace[0], "rv": trace[1], "wv": trace[2], "proof": proof.hex()}


def main():
    ss = [int(x, 16) for x in json.load(open(os.path.join(HERE, "lasso_tables.json")))["srs"]["ss"]]
    pps = {False: kzg.setup(ss), True: None}
    out = {"mid_srs_seed": lgr.MID_SRS_SEED, "cases": {}, "chain": [], "forgeries": {}}
    for case, (n, l) in msr.CASES.items():
        big = case not in msr.SMALL
        if big and pps[True] is None:
            pps[True] = kzg.setup(lgr.mid_ss())
        out["cases"][case], _ = segment(pps[big], n, l, msr.case_trace(case), msr.case_image(case))
    n, l, _ = msr.CHAIN
    traces, images = msr.chain_traces()
    for k, trace in enumerate(traces):
        rec, fv = segment(pps[False], n, l, trace, images[k])
        assert fv == images[k + 1]
        out["chain"].append(rec)
    for a, b in zip(out["chain"], out["chain"][1:]):
        assert a["final_commitment"] == b["image_commitment"]
    for name in msr.FORGERIES:
        out["forgeries"][name] = forged(pps[False], name)
    with open(os.path.join(HERE, "memcheck_segment.json"), "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()
