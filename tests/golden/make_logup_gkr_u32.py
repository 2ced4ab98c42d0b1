"""Regenerate tests/golden/logup_gkr_u32.json: LogUp-GKR proofs whose input columns are (some or all) 32-bit words, from
the UNCHANGED specification tests/logup_gkr_ref.py - a u32 column and the same values as field elements are the same
polynomial, so the specification knows nothing about kinds.

    python tests/golden/make_logup_gkr_u32.py

A u32 column is a column whose table values are drawn below 2^32.  The SRS secrets of the cases up to six variables are
tests/golden/lasso_tables.json's; `u32_mid` uses the seeded 14 secrets of logup_gkr_ref.mid_ss().  Records, for every
case, its shape, the kind of every column (1: u32), the table row of every input row and the proof (tables and inputs
follow from the case's seeds: case_tables / case_rows below, which the tests import).  The specification's own verifier
accepts every proof before it is written.  `u32_mid` takes about half a minute.
"""
import json
import os
import random
import sys
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import logup_gkr_ref as lgr  # noqa: E402
from oracle.pyref import kzg  # noqa: E402
from oracle.pyref.field import R_MOD as P  # noqa: E402
from oracle.pyref.transcript import Keccak256Transcript as T  # noqa: E402

# the named cases: (n, l, per lookup the kind of every column - 1: uint32_t, 0: Fr)
CASES = {
    "u32_one_var": (1, 1, [[1]]),               # the leaves are the top layer; widen-only compress
    "u32_mixed": (5, 3, [[1, 0, 1], [0]]),      # a mixed row, commitment order, evaluation order
    "u32_big_table": (2, 4, [[1, 1]]),          # nv > n: no padding, level-nv bases with 2^n scalars
    "u32_edges": (4, 3, [[1]]),                 # 0, 1, 2^16, 2^31, 2^32 - 1, each looked up: known_bits = 32, Wide carries
    "u32_zeros": (4, 3, [[1]]),                 # the identity commitment, the known_bits clamp
    "u32_wide": (6, 6, [[1] * 8]),              # LOGUP_MAX columns in the kernel arguments
    "u32_mid": (13, 9, [[1, 1], [1]]),          # many workgroups, the grid-stride tail
}
SMALL = [c for c in CASES if max(CASES[c][:2]) <= 6]
EDGES = [0, 1, 1 << 16, 1 << 31, (1 << 32) - 1]


def _rng(case, what):
    return random.Random(zlib.crc32(repr((case, what)).encode()))


def case_tables(case):
    """per lookup its columns of 2^l seeded values: below 2^32 in a u32 column, field elements in an Fr column"""
    n, l, kinds = CASES[case]
    rng = _rng(case, "table")
    M = 1 << l
    tables = [[[rng.randrange(1 << 32) if kind else rng.randrange(P) for _ in range(M)] for kind in ks] for ks in kinds]
    if case == "u32_edges":
        tables[0][0][:len(EDGES)] = EDGES
    if case == "u32_zeros":
        tables = [[[0] * M]]
    return tables


def case_rows(case):
    """per lookup the table row of every input row"""
    n, l, kinds = CASES[case]
    rng = _rng(case, "rows")
    rows = [[rng.randrange(1 << l) for _ in range(1 << n)] for _ in kinds]
    if case == "u32_edges":  # every edge value is looked up, the largest next to the smallest
        rows[0][:6] = [4, 0, 1, 2, 3, 4]
    return rows


def case_lookups(case):
    tables = case_tables(case)
    return list(zip(lgr.inputs_of(tables, case_rows(case)), tables))


def generate(cases=None):
    """the file's content (cases: a subset of the names, for a test that has no half minute to spend on `u32_mid`)"""
    ss = [int(x, 16) for x in json.load(open(os.path.join(HERE, "lasso_tables.json")))["srs"]["ss"]]
    pps = {False: kzg.setup(ss), True: None}
    out = {"mid_srs_seed": lgr.MID_SRS_SEED, "cases": {}}
    for case, (n, l, kinds) in CASES.items():
        if cases is not None and case not in cases:
            continue
        big = case not in SMALL
        if big and pps[True] is None:
            pps[True] = kzg.setup(lgr.mid_ss())
        pp = pps[big]
        lookups = case_lookups(case)
        assert all(v < 1 << 32 for (f, _), ks in zip(lookups, kinds) for col, kind in zip(f, ks) if kind for v in col)
        t = T()
        lgr.prove(pp, lookups, t)
        proof = t.into_proof()
        lgr.verify(pp, [tb for _, tb in lookups], n, T(proof))
        out["cases"][case] = {"n": n, "l": l, "widths": [len(ks) for ks in kinds], "kinds": kinds, "rows": case_rows(case),
                              "proof": proof.hex()}
    return out


def dump(out):
    return json.dumps(out, indent=0) + "\n"


def main():
    with open(os.path.join(HERE, "logup_gkr_u32.json"), "w") as f:
        f.write(dump(generate()))


if __name__ == "__main__":
    main()
