"""Lasso and HyperPlonk over the Ligero PCS, restated: the oracle's provers (oracle/pyref/lasso.py, oracle/pyref/hyperplonk.py,
generic over their PCS) run over tests/ligero_ref.py through the adapter of tests/brakedown_provers_ref.py with the other
PCS module in it.  The transcripts are brakedown_provers_ref's and brakedown_lasso_ref's: roots are hashes, raw stream bytes.

Unlike over Spec6 (3 755 columns per opening) an opening here is 309 columns at rate 1/4, so the oracle's proofs are made in
the tests themselves, in a second or two, and nothing is recorded."""
import random

import brakedown_lasso_ref as bl
import brakedown_provers_ref as bp
import hyrax_provers_ref as hr
import ligero_ref as lr
from oracle.pyref import hyperplonk as o_hp
from oracle.pyref import lasso as o_lasso

LOG_INV_RATE = 2
LASSO_CASE = ("range", 2, 4, 8)   # kind, c, l, n: a range table of 2 chunks of 4 bits, 2^8 lookups
HYPERPLONK_VARS = 6               # vanilla_plonk_with_lookup at 2^6 rows


class LigeroPcs(bp.BrakedownPcs):
    """brakedown_provers_ref.BrakedownPcs with ligero_ref's commit, open and verify"""

    def commit(self, pp, poly):
        key = tuple(poly)
        if key not in self.comms:
            self.comms[key] = lr.commit(pp, list(poly))
        return self.comms[key]

    def batch_open(self, pp, num_vars, polys, points, evals, transcript):
        for e in evals:
            poly = polys[e.poly]
            lr.open_(pp, poly, self.comms[tuple(poly)], points[e.point], transcript)

    def batch_verify(self, vp, num_vars, comms, points, evals, transcript):
        for e in evals:
            c = comms[e.poly]
            lr.verify(vp, c if isinstance(c, bytes) else c.root, points[e.point], e.value, transcript)


def lasso_case():
    """-> (oracle table spec, dims, num_vars of the lookups, num_vars of the param)"""
    kind, c, l, n = LASSO_CASE
    spec, dims, _, _ = hr.lasso_case(kind, c, l, n, 1)
    return spec, dims, n, max(n, l)


def lasso_prove():
    spec, dims, n, nv = lasso_case()
    pp = lr.Params(nv, LOG_INV_RATE)
    tr = bl.Transcript()
    o_lasso.prove(pp, spec, dims, tr, LigeroPcs())
    return tr.into_proof()


def hyperplonk_circuit():
    """-> (oracle info, instances, witness tables)"""
    info, instances, witness = o_hp.rand_vanilla_plonk_with_lookup_circuit(HYPERPLONK_VARS, random.Random(bp.SEED))
    return info, instances, witness


def hyperplonk_prove():
    """-> (proof bytes, preprocess roots, permutation roots)"""
    info, instances, witness = hyperplonk_circuit()
    pp = lr.Params(HYPERPLONK_VARS, LOG_INV_RATE)
    pcs = LigeroPcs()
    o_pp = o_hp.preprocess((pp, pp), info, pcs)
    tr = bp.Transcript()
    o_hp.prove(o_pp, instances, lambda rnd, challenges: witness, tr)
    return tr.into_proof(), [c.root for c in o_pp.preprocess_comms], [c.root for c in o_pp.permutation_comms]
