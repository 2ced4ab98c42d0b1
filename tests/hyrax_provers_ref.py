"""Restatement of Lasso over MultilinearHyrax, byte for byte: the chunked commitment framing and prove / verify built from
the oracle's witness / argue / check (oracle/pyref/lasso.py) and the Hyrax restatement of tests/ipa_ref.py.

Framing (include/lasso_hip.h, lh_lasso_prove_hyrax): the count commitments of num_chunks points each are flattened
commitment-major; ceil(total / 63) mask field elements come first, mask k covering the flat positions 63 k .. 63 k + 62 with
bit i = "position 63 k + i is the identity"; then the non-identity points in order.  With num_chunks = 1 (count <= 63) this is
oracle.pyref.lasso.write_commitments bit for bit."""
import ipa_ref as ir
from oracle.pyref import lasso as o_lasso

MASK_BITS = 63


def write_commitments(transcript, comms):
    """comms: a list of commitments, each a list of num_chunks points (None = identity)"""
    flat = [p for cm in comms for p in cm]
    for k in range(0, len(flat), MASK_BITS):
        transcript.write_field_element(sum(1 << i for i, p in enumerate(flat[k:k + MASK_BITS]) if p is None))
    transcript.write_commitments([p for p in flat if p is not None])
    return flat


def read_commitments(transcript, count, chunks):
    total = count * chunks
    masks = []
    for k in range(0, total, MASK_BITS):
        m = transcript.read_field_element()
        if m >> min(MASK_BITS, total - k):
            raise o_lasso.LassoError("commitment mask out of range")
        masks.append(m)
    flat = [None if (masks[i // MASK_BITS] >> (i % MASK_BITS)) & 1 else transcript.read_commitment() for i in range(total)]
    return [flat[i * chunks:(i + 1) * chunks] for i in range(count)]


def params(n_vars, batch_size):
    """-> (pp, vp) of the oracle for tables of 2^n_vars entries"""
    return ir.hyrax_trim(ir.hyrax_setup(1 << n_vars, batch_size), 1 << n_vars, batch_size)


def prove(pp, spec, dims, transcript):
    c, l, alpha = spec.c, spec.l, spec.alpha
    n = len(dims[0]).bit_length() - 1
    w = o_lasso.witness(spec, dims)
    transcript.common_field_elements([n, l, c, alpha])
    nv = max(n, l)
    assert nv == pp.num_vars
    polys = [o_lasso._pad(p, nv) for p in [w["a"]] + w["dim"] + w["read_ts"] + w["E"] + w["final_cts"]]
    flat = write_commitments(transcript, [ir.hyrax_commit(pp, p) for p in polys])
    pts, vals = o_lasso.argue(spec, w, transcript)
    ir.hyrax_batch_open(pp, nv, polys, [o_lasso._pad_point(pt, nv) for pt in pts], o_lasso._evals(spec, *vals), transcript)
    return flat


def verify(vp, spec, n, transcript):
    c, l, alpha = spec.c, spec.l, spec.alpha
    transcript.common_field_elements([n, l, c, alpha])
    nv = max(n, l)
    comms = read_commitments(transcript, 1 + 3 * c + alpha, vp.num_chunks)
    pts, vals = o_lasso.check(spec, n, transcript)
    ir.hyrax_batch_verify(vp, nv, comms, [o_lasso._pad_point(pt, nv) for pt in pts], o_lasso._evals(spec, *vals), transcript)
    if transcript.pos != len(transcript.stream):
        raise o_lasso.LassoError("trailing bytes in proof")


# the issue's four inputs: (kind, c, l, n, batch_size) -> (chunks, points, identities, masks, proof bytes)
LASSO_CASES = [("range", 2, 3, 4, 1), ("and", 2, 4, 3, 1), ("xor", 2, 4, 6, 1), ("range", 2, 2, 6, 4)]
LASSO_SHAPES = {("range", 2, 3, 4, 1): (4, 36, 4, 1, 6304), ("and", 2, 4, 3, 1): (4, 36, 16, 1, 5440),
                ("xor", 2, 4, 6, 1): (8, 72, 12, 2, 10560), ("range", 2, 2, 6, 4): (4, 36, 6, 1, 8224)}


def lasso_case(kind, c, l, n, batch_size):
    """-> (spec, dims, oracle pp, oracle vp) with the draws of test_lasso_over_ipa_matches_oracle"""
    import random
    rng = random.Random(700 + n)
    spec = o_lasso.range_table(c, l) if kind == "range" else o_lasso.bitwise_table(
        o_lasso.SUBTABLE_AND if kind == "and" else o_lasso.SUBTABLE_XOR, c, l)
    dims = [[rng.randrange(1 << l) for _ in range(1 << n)] for _ in range(c)]
    pp, vp = params(max(n, l), batch_size)
    return spec, dims, pp, vp


_proofs = {}


def lasso_proof(case):
    """the restatement's proof of a case (computed once per process) -> (proof bytes, flat commitment points)"""
    if case not in _proofs:
        from oracle.pyref.transcript import Keccak256Transcript as OT
        spec, dims, pp, _ = lasso_case(*case)
        ot = OT()
        flat = prove(pp, spec, dims, ot)
        _proofs[case] = (ot.into_proof(), flat)
    return _proofs[case]


# ------------------------------------------------------------------ HyperPlonk over Hyrax: what the oracle needs from a PCS
class HyraxPcs:
    """the PolynomialCommitmentScheme object oracle.pyref.hyperplonk.preprocess(..., pcs_mod) is generic over, with
    MultilinearHyrax underneath: a commitment is the list of num_chunks row commitments"""
    commit = staticmethod(ir.hyrax_commit)
    batch_commit_and_write = staticmethod(ir.hyrax_batch_commit_and_write)
    batch_open = staticmethod(ir.hyrax_batch_open)
    batch_verify = staticmethod(ir.hyrax_batch_verify)


def chunked_transcript(num_chunks):
    """a Keccak256Transcript whose read_commitments(n) returns n commitments of num_chunks points (the oracle's verify reads
    the witness, m, h and z commitments through it)"""
    from oracle.pyref.transcript import Keccak256Transcript as OT

    class ChunkedTranscript(OT):
        def read_commitments(self, n):
            flat = OT.read_commitments(self, n * num_chunks)
            return [tuple(flat[i * num_chunks:(i + 1) * num_chunks]) for i in range(n)]
    return ChunkedTranscript


def patch_lasso_framing(monkeypatch, num_chunks):
    """HyperPlonk's Lasso lookups: the oracle frames their commitments through oracle.pyref.lasso's two functions"""
    monkeypatch.setattr(o_lasso, "write_commitments", lambda t, comms: write_commitments(t, comms))
    monkeypatch.setattr(o_lasso, "read_commitments", lambda t, count: read_commitments(t, count, num_chunks))


# the issue's inputs: (num_vars, batch_size, with_lookup, seed) -> (chunks, proof bytes)
HP_CASES = [(5, 1, False, 1), (5, 1, True, 2), (6, 4, True, 3)]
HP_SHAPES = {(5, 1, False, 1): (4, 3328), (5, 1, True, 2): (4, 4032), (6, 4, True, 3): (4, 4448)}
_hp = {}


def hp_case(case):
    """-> (oracle info, instances, witness, oracle prover param, proof) of a case, computed once per process"""
    if case not in _hp:
        import random
        from oracle.pyref import hyperplonk as o_hp
        from oracle.pyref.transcript import Keccak256Transcript as OT
        num_vars, batch_size, with_lookup, seed = case
        gen = o_hp.rand_vanilla_plonk_with_lookup_circuit if with_lookup else o_hp.rand_vanilla_plonk_circuit
        o_info, instances, witness = gen(num_vars, random.Random(seed))
        o_pp = o_hp.preprocess(params(num_vars, batch_size), o_info, HyraxPcs)
        ot = OT()
        o_hp.prove(o_pp, instances, lambda rnd, ch: witness, ot)
        _hp[case] = (o_info, instances, witness, o_pp, ot.into_proof())
    return _hp[case]
