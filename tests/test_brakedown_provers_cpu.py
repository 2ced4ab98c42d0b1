"""CPU: HyperPlonk over Brakedown.  The fixture tests/golden/brakedown_hyperplonk.json against the restatement that wrote it
(tests/brakedown_provers_ref.py: the oracle's prover over tests/brakedown_ref.py) - case (a) proved again (~20 s: 14
evaluations of 3 755 columns each, the one slow test here), the cases' shapes from the parameters - and the boundary: the
header declares the four entries and the built library exports them.  The oracle's verifier takes minutes on the smallest
case and is run nowhere."""
import ctypes as C
import hashlib
import os
import re

import brakedown_provers_ref as bp
import brakedown_ref as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["lh_hyperplonk_prove_brakedown", "lh_hyperplonk_prove_phases_brakedown", "lh_hyperplonk_verify_brakedown",
           "lh_hyperplonk_verify_phases_brakedown"]


def test_case_a_is_what_the_oracle_proves():
    fx = bp.fixture()["a"]
    proof, pre, perm, num_evals = bp.oracle_prove(bp.cases()["a"])
    assert len(proof) == fx["proof_len"] == 8415936
    assert hashlib.sha256(proof).hexdigest() == fx["proof_sha256"]
    assert [r.hex() for r in pre] == fx["preprocess_roots"] and [r.hex() for r in perm] == fx["permutation_roots"]
    assert num_evals == fx["num_evaluations"] == 14


def test_the_cases_and_their_shapes():
    fx, cases = bp.fixture(), bp.cases()
    assert sorted(fx) == ["a", "b", "c"]
    for name, case in cases.items():
        rec = fx[name]
        assert rec["case"] == [case[0], case[1], case[2], list(case[3])]
        p = br.Params(case[0], case[1])
        assert (rec["num_rows"], rec["codeword_len"], rec["num_column_opening"]) == (p.num_rows, p.codeword_len,
                                                                                       p.num_column_opening)
        # the proof's length from its parts: instances are not written; roots, the zero-check's messages, the evaluations,
        # then per evaluation the combined rows and the opened columns with their paths
        rows = (p.num_proximity_testing + 1) * p.row_len if p.num_rows > 1 else p.row_len
        one_open = 32 * (rows + p.num_column_opening * (p.num_rows + p.depth))
        assert rec["proof_len"] > rec["num_evaluations"] * one_open
        assert (rec["proof_len"] - rec["num_evaluations"] * (one_open + 32)) % 32 == 0
    # (a): one row, the codeword of 14; (b): the first size with more than one row, and the spec that opens the fewest columns
    assert (fx["a"]["num_rows"], fx["a"]["codeword_len"], fx["a"]["num_column_opening"]) == (1, 14, 3755)
    assert fx["b"]["num_rows"] > 1 and br.Params(cases["b"][0] - 1, cases["b"][1]).num_rows == 1
    # splitting the witness over two phases squeezes nothing in between: the same roots in the same order, the same proof
    assert fx["c"]["proof_sha256"] == fx["b"]["proof_sha256"] and cases["c"][3] == [2, 1]


def test_the_four_entries_are_declared_and_exported(hl):
    from halo2_lasso_amd import _ffi
    header = open(os.path.join(ROOT, "include", "lasso_hip.h")).read()
    lib = _ffi.load()
    for name in ENTRIES:
        assert re.search(r"\blh_status\s+%s\s*\(" % name, header), name
        assert isinstance(getattr(lib, name), C._CFuncPtr) and name in _ffi.SIGNATURES
    # NULL arguments are statuses (host-only entries: no GPU needed)
    prm = _ffi.lh_hp_vparam()
    assert lib.lh_hyperplonk_verify_brakedown(None, C.byref(prm), None, None, None, None, None) == _ffi.LH_ERR_ARG
    assert lib.lh_hyperplonk_verify_phases_brakedown(None, None, None, None, 0, None, None, None, None, None) == _ffi.LH_ERR_ARG
    vp = hl.BrakedownVerifierParam.derive(3, 6)
    assert lib.lh_hyperplonk_verify_brakedown(vp.h, None, None, None, None, None, None) == _ffi.LH_ERR_ARG
    t = hl.Keccak256Transcript()
    prm.num_vars = 3
    assert lib.lh_hyperplonk_verify_brakedown(vp.h, C.byref(prm), None, None, None, t.p, None) == _ffi.LH_ERR_ARG
    prm.num_vars, prm.num_preprocess_polys = 4, 0  # a circuit of another size than the param's
    assert lib.lh_hyperplonk_verify_brakedown(vp.h, C.byref(prm), None, None, None, t.p, C.byref(t.hash_io())) == _ffi.LH_ERR_ARG
    assert b"variables" in lib.lh_last_error()
