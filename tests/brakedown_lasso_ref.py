"""Lasso over MultilinearBrakedown, restated: the oracle's prover (oracle/pyref/lasso.py, generic over its PCS) run over the
Brakedown adapter of tests/brakedown_provers_ref.py, and the cases of tests/golden/brakedown_lasso.json.

lasso.write_commitments writes one mask field element (here always zero: the adapter's commitment of the zero column is an
object with a root like any other, never None) and hands the commitments to transcript.write_commitments; lasso.verify reads
them back one by one through read_commitment.  Over Brakedown both are hashes: raw stream bytes, not absorbed.  E_i of an
identity subtable is the same table as dim_j, so the adapter (which remembers commitments by their table) commits it once
and its root is written twice.

The oracle's cost is that of brakedown_provers_ref: 3 755 opened columns per evaluation at every size under Spec6, so a proof
is 4-20 MB and takes 7-20 s to make; its verification takes over a minute and no test runs it.  The GPU tests compare against
the recorded length, digest and roots of the fixture, which tests/golden/make_brakedown_lasso.py writes."""
import hashlib
import json
import os

import brakedown_provers_ref as bp
import brakedown_ref as br
import hyrax_provers_ref as hr
from oracle.pyref import lasso as o_lasso

SEED = bp.SEED
SPEC = 6
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "brakedown_lasso.json")


class Transcript(bp.Transcript):
    def write_commitments(self, comms):
        for c in comms:
            self.write_hash(c.root)

    def read_commitment(self):
        return self.read_hash()


# name -> (kind, c, l, n, pinned dims per chunk or None: drawn as hyrax_provers_ref.lasso_case draws them)
_NO_COMMON_BIT = [(x << 2) | y for x, y in [(0, 0), (1, 2), (2, 1), (3, 0), (0, 3), (1, 0), (2, 0), (0, 1)]]
CASES = {
    "a": ("range", 2, 3, 4, None),                     # one row, n > l, identity subtables (a root written twice)
    "b": ("and", 2, 4, 3, {0: _NO_COMMON_BIT}),        # one row, n < l; E_0 is all zero (operands without a common bit)
    "c": ("xor", 1, 4, 2, {0: [3, 9, 12, 5]}),         # pairwise distinct indices: read_ts identically zero
    "d": ("xor", 2, 8, 4, None),                       # g with more than one term, columns of known_bits 4
    "e": ("range", 2, 2, 12, None),                    # two rows of 2048; final_cts occupies 4 entries: a row is all padding
    "f": ("and", 1, 12, 3, None),                      # two rows; the lookup columns are the padded ones
}


def case(name):
    """-> (oracle table spec, dims, num_vars of the lookups, num_vars of the param)"""
    kind, c, l, n, pinned = CASES[name]
    spec, dims, _, _ = hr.lasso_case(kind, c, l, n, 1)
    for j, col in (pinned or {}).items():
        assert len(col) == 1 << n and all(0 <= d < 1 << l for d in col)
        dims[j] = list(col)
    return spec, dims, n, max(n, l)


def oracle_prove(name):
    """-> (proof bytes, the 1 + 3 c + alpha roots in the order they were written, number of evaluations)"""
    spec, dims, n, nv = case(name)
    pp = br.Params(nv, SPEC, SEED)
    pcs = bp.BrakedownPcs()
    written, counted = [], []

    class Recording(Transcript):
        def write_commitments(self, comms):
            written.extend(c.root for c in comms)
            super().write_commitments(comms)
    inner = pcs.batch_open

    def batch_open(p, num_vars, polys, points, evals, transcript):
        counted.append(len(evals))
        inner(p, num_vars, polys, points, evals, transcript)
    pcs.batch_open = batch_open
    tr = Recording()
    o_lasso.prove(pp, spec, dims, tr, pcs)
    assert len(written) == 1 + 3 * spec.c + spec.alpha and counted == [1 + 3 * spec.c + 2 * spec.alpha]
    return tr.into_proof(), written, counted[0]


def record(name):
    proof, roots, num_evals = oracle_prove(name)
    kind, c, l, n, _ = CASES[name]
    p = br.Params(max(n, l), SPEC)
    return {"case": [kind, c, l, n], "num_vars": max(n, l), "spec": SPEC, "num_rows": p.num_rows, "row_len": p.row_len,
            "codeword_len": p.codeword_len, "num_column_opening": p.num_column_opening, "num_evaluations": num_evals,
            "proof_len": len(proof), "proof_sha256": hashlib.sha256(proof).hexdigest(), "roots": [r.hex() for r in roots]}


def fixture():
    with open(FIXTURE) as f:
        return json.load(f)
