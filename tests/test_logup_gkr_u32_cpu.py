"""CPU: LogUp-GKR from 32-bit input columns (lh_logup_gkr_prove_columns, hl.U32Column) - what needs no device.  The golden
proofs (tests/golden/logup_gkr_u32.json) come from the unchanged specification (tests/logup_gkr_ref.py): the generator
reproduces them, the host verifier accepts them through the plain lookup list, the library exports the entry, and the
Python wrapper refuses a u32 column of the wrong shape before a ctx exists."""
import importlib.util
import json
import os

import pytest

import logup_gkr_ref as lgr

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_logup_gkr_u32", os.path.join(HERE, "golden", "make_logup_gkr_u32.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)
GOLDEN = json.load(open(os.path.join(HERE, "golden", "logup_gkr_u32.json")))
SS = [int(x, 16) for x in json.load(open(os.path.join(HERE, "golden", "lasso_tables.json")))["srs"]["ss"]]


@pytest.fixture(scope="module")
def vps(hl):
    return {True: hl.MultilinearKzgVerifierParams.setup(SS), False: hl.MultilinearKzgVerifierParams.setup(lgr.mid_ss())}


def test_the_generator_reproduces_the_committed_file():
    """every case up to six variables is proved again by the specification (`u32_mid` takes it half a minute: its shape,
    kinds and rows are compared here and its proof goes through the host verifier below)"""
    assert list(GOLDEN["cases"]) == list(gen.CASES) and GOLDEN["mid_srs_seed"] == lgr.MID_SRS_SEED
    assert gen.SMALL == [c for c in gen.CASES if c != "u32_mid"]
    again = gen.generate(gen.SMALL)
    for case, (n, l, kinds) in gen.CASES.items():
        g = GOLDEN["cases"][case]
        assert (g["n"], g["l"], g["kinds"], g["widths"]) == (n, l, kinds, [len(ks) for ks in kinds]), case
        assert g["rows"] == gen.case_rows(case), case
        if case in gen.SMALL:
            assert again["cases"][case] == g, case + ": the golden bytes are not what the specification produces now"
    small_only = dict(GOLDEN, cases={c: GOLDEN["cases"][c] for c in gen.SMALL})
    assert gen.dump(again) == gen.dump(small_only)


def test_the_cases_hold_what_they_are_named_for():
    for case, (n, l, kinds) in gen.CASES.items():
        for (f, t), ks in zip(gen.case_lookups(case), kinds):
            for col, tcol, kind in zip(f, t, ks):
                assert not kind or max(col + tcol) < 1 << 32, case
    (f, t), = gen.case_lookups("u32_edges")
    assert t[0][:5] == gen.EDGES == [0, 1, 1 << 16, 1 << 31, (1 << 32) - 1] and set(gen.EDGES) <= set(f[0])
    (f, t), = gen.case_lookups("u32_zeros")
    assert not any(f[0]) and not any(t[0])
    assert gen.CASES["u32_wide"][2] == [[1] * lgr.MAX_WIDTH]
    assert any(0 in ks and 1 in ks for ks in gen.CASES["u32_mixed"][2])
    # the all-zero input column commits to the identity: bit 0 of the first mask (its repr is big-endian)
    assert int.from_bytes(bytes.fromhex(GOLDEN["cases"]["u32_zeros"]["proof"])[:32], "big") == 1


@pytest.mark.parametrize("case", list(gen.CASES))
def test_host_verifier_accepts_golden_and_refuses_a_damaged_commitment(hl, vps, case):
    n = gen.CASES[case][0]
    proof = bytes.fromhex(GOLDEN["cases"][case]["proof"])
    statement = [hl.LogupLookup(None, t) for t in gen.case_tables(case)]
    tr = hl.Keccak256Transcript.from_proof(proof)
    hl.logup_gkr_verify(vps[case in gen.SMALL], statement, n, tr)
    assert tr.remaining() == 0
    # a flipped byte in a commitment: the first point behind the input mask, or - when every input commitment is the
    # identity and the block is the mask alone - the first point of the multiplicities' block
    mask = int.from_bytes(proof[:32], "big")
    W = sum(len(ks) for ks in gen.CASES[case][2])
    points = W - bin(mask).count("1")
    pos = 32 + 3 if points else 32 + 32 + 3
    bad = bytearray(proof)
    bad[pos] ^= 4
    with pytest.raises(hl.InvalidSnark):
        hl.logup_gkr_verify(vps[case in gen.SMALL], statement, n, hl.Keccak256Transcript.from_proof(bytes(bad)))


def test_the_library_exports_the_entry_and_the_constants(hl):
    from halo2_lasso_amd import _ffi
    lib = _ffi.load()
    assert hasattr(lib, "lh_logup_gkr_prove_columns")
    assert (_ffi.LH_LOGUP_COL_FR, _ffi.LH_LOGUP_COL_U32) == (0, 1)
    header = open(os.path.join(os.path.dirname(HERE), "include", "lasso_hip.h")).read()
    assert "#define LH_LOGUP_COL_FR  0" in header and "#define LH_LOGUP_COL_U32 1" in header
    assert "lh_status lh_logup_gkr_prove_columns(" in header
    # as far as the entry gets without a device: NULL ctx, and never a crash on NULL lists
    arr = (_ffi.lh_logup_columns * 1)()
    assert lib.lh_logup_gkr_prove_columns(None, None, arr, 1, 4, 3, None) == _ffi.LH_ERR_ARG
    assert lib.lh_logup_gkr_prove_columns(None, None, None, 1, 4, 3, None) == _ffi.LH_ERR_ARG


def test_u32_column_refusals_need_no_ctx(hl):
    col = gen.case_tables("u32_edges")[0][0]
    buf = lambda nbytes: hl.DeviceBuffer(None, nbytes, ptr=0x1000)  # (a buffer that is never touched)
    prove = lambda inputs, n: hl.logup_gkr_prove(None, [hl.LogupLookup(inputs, [col])], hl.Keccak256Transcript(), n)
    with pytest.raises(hl.ArgumentError, match="2\\^num_vars"):  # the column's num_vars against the proof's
        prove([hl.U32Column(buf(4 << 4), 4)], 5)
    with pytest.raises(hl.ArgumentError, match="bytes"):  # a buffer shorter than 4 * 2^n bytes
        prove([hl.U32Column(buf((4 << 4) - 4), 4)], 4)
    with pytest.raises(hl.ArgumentError, match="bytes"):  # ... also when num_vars comes from the column itself
        prove([hl.U32Column(buf(8), 4)], None)
    with pytest.raises(hl.ArgumentError):  # a mixed lookup: the Fr column disagrees
        hl.logup_gkr_prove(None, [hl.LogupLookup([hl.U32Column(buf(4 << 4), 4), hl.MultilinearPolynomial(None, buf(32 << 3), 3)],
                                                 [col, col])], hl.Keccak256Transcript(), 4)
