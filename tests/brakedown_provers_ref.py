"""HyperPlonk over MultilinearBrakedown, restated: the glue between the oracle's prover (oracle/pyref/hyperplonk.py, generic
over its PCS) and the Brakedown restatement of tests/brakedown_ref.py, and the cases of tests/golden/brakedown_hyperplonk.json.

A Brakedown commitment is the encoded rows plus the Merkle tree, and its opening needs it; the oracle's batch_open is handed
polys only, so the adapter remembers the commitment of every table it committed.  A commit round writes the 32-byte roots
through write_hash: raw stream bytes, not absorbed (util/transcript.rs:240-265).  batch_open is one open per evaluation, in
order (pcs/multilinear/brakedown.rs:278-300).

The oracle's cost: every open writes num_column_opening columns (3 755 for Spec6) at every size, so a proof of the smallest
circuit is 8 MB and takes ~20 s to make; its verification takes minutes and no test runs it.  The GPU tests compare against
the recorded length and digest of the fixture, which tests/golden/make_brakedown_hyperplonk.py writes."""
import hashlib
import json
import os
import random

import brakedown_ref as br
from oracle.pyref import hyperplonk as o_hp

SEED = bytes(range(7, 39))
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "brakedown_hyperplonk.json")


class BrakedownPcs:
    """the PolynomialCommitmentScheme object oracle.pyref.hyperplonk.preprocess(..., pcs_mod) is generic over"""

    def __init__(self):
        self.comms = {}

    def commit(self, pp, poly):
        key = tuple(poly)
        if key not in self.comms:
            self.comms[key] = br.commit(pp, list(poly))
        return self.comms[key]

    def batch_commit_and_write(self, pp, polys, transcript):
        comms = [self.commit(pp, p) for p in polys]
        for c in comms:
            transcript.write_hash(c.root)
        return comms

    def batch_open(self, pp, num_vars, polys, points, evals, transcript):
        for e in evals:
            poly = polys[e.poly]
            br.open_(pp, poly, self.comms[tuple(poly)], points[e.point], transcript)

    def batch_verify(self, vp, num_vars, comms, points, evals, transcript):
        for e in evals:
            c = comms[e.poly]
            br.verify(vp, c if isinstance(c, bytes) else c.root, points[e.point], e.value, transcript)


class Transcript(br.Transcript):
    """the oracle's verify reads the witness, m, h and z commitments through read_commitments: here they are hashes"""

    def read_commitments(self, n):
        return [self.read_hash() for _ in range(n)]


def smallest_multi_row():
    """-> (num_vars, spec): the smallest num_vars at which some spec's parameters have num_rows > 1, and among the specs
    1..6 that do at that size the one with the fewest column openings (ties: the lowest number)"""
    for nv in range(1, 33):
        best = None
        for spec in range(1, 7):
            try:
                p = br.Params(nv, spec)
            except (br.PcsError, AssertionError, ValueError, ZeroDivisionError):
                continue  # (the smallest sizes have no valid code under some specs: the reference panics there)
            if p.num_rows > 1 and (best is None or p.num_column_opening < best[0]):
                best = (p.num_column_opening, spec)
        if best:
            return nv, best[1]
    raise AssertionError("no multi-row parameters")


def cases():
    """-> {name: (num_vars, spec, with_lookup, phases)}; phases: the witness polys per phase"""
    nv, spec = smallest_multi_row()
    return {"a": (3, 6, False, [3]), "b": (nv, spec, True, [3]), "c": (nv, spec, True, [2, 1])}


def circuit(case):
    """-> (oracle info, instances, witness_fn) of a case tuple; a split of the witness polys over phases squeezes no
    challenge in between, so synthesize hands out the same three tables in slices"""
    num_vars, _, with_lookup, phases = case
    gen = o_hp.rand_vanilla_plonk_with_lookup_circuit if with_lookup else o_hp.rand_vanilla_plonk_circuit
    info, instances, witness = gen(num_vars, random.Random(SEED))
    info.num_witness_polys, info.num_challenges = list(phases), [0] * len(phases)
    starts = [sum(phases[:r]) for r in range(len(phases))]
    return info, instances, lambda rnd, challenges: witness[starts[rnd]:starts[rnd] + phases[rnd]]


def oracle_prove(case):
    """-> (proof bytes, preprocess roots, permutation roots, number of evaluations) by the oracle's prover"""
    num_vars, spec = case[0], case[1]
    info, instances, witness_fn = circuit(case)
    pp = br.Params(num_vars, spec, SEED)
    pcs = BrakedownPcs()
    o_pp = o_hp.preprocess((pp, pp), info, pcs)
    tr = Transcript()
    counted = []
    inner = pcs.batch_open

    def batch_open(p, nv, polys, points, evals, transcript):
        counted.append(len(evals))
        inner(p, nv, polys, points, evals, transcript)
    pcs.batch_open = batch_open
    o_hp.prove(o_pp, instances, witness_fn, tr)
    return (tr.into_proof(), [c.root for c in o_pp.preprocess_comms], [c.root for c in o_pp.permutation_comms], counted[0])


def record(case):
    proof, pre, perm, num_evals = oracle_prove(case)
    p = br.Params(case[0], case[1])
    return {"case": [case[0], case[1], case[2], list(case[3])], "num_rows": p.num_rows, "codeword_len": p.codeword_len,
            "num_column_opening": p.num_column_opening, "num_evaluations": num_evals, "proof_len": len(proof),
            "proof_sha256": hashlib.sha256(proof).hexdigest(), "preprocess_roots": [r.hex() for r in pre],
            "permutation_roots": [r.hex() for r in perm]}


def fixture():
    with open(FIXTURE) as f:
        return json.load(f)
