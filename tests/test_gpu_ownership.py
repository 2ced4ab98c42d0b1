"""GPU: who owns the device resources (csrc/owned.hpp).  A context that has created all of its lazy state, and every kind of
param and commitment made through it, give everything back - counted by lh_debug_live_resources -; freeing on another
device leaves the caller's device current; a creation entry that fails half-way (lh_debug_fail_acquire_after) holds
nothing afterwards and works the next time.  Every test uses a context of its own."""
import array
import ctypes as C
import gc
import hashlib
import json
import os
import random

import pytest

import spark_ref as spr
import spartan_ref as spa
import test_gpu_hyperplonk as thp
from oracle.pyref.field import R_MOD as P

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SS = [int(x, 16) for x in json.load(open(os.path.join(HERE, "golden", "lasso_tables.json")))["srs"]["ss"]]
SEED = bytes(range(32))


def _live(lib):
    out = (C.c_uint64 * 4)()
    assert lib.lh_debug_live_resources(out) == 0
    return tuple(out)


def _polys(hl, ctx, rng, count, nv):
    return [hl.MultilinearPolynomial.new(ctx, [rng.randrange(P) for _ in range(1 << nv)]) for _ in range(count)]


# ------------------------------------------------------------------ 1. balance
def test_everything_a_context_made_goes_back(hl):
    from halo2_lasso_amd import _ffi
    lib = _ffi.load()
    gc.collect()  # (handles of earlier tests that nobody freed go now, not in the middle of the count)
    before = _live(lib)
    rng = random.Random(61)
    ctx = hl.Context(0)

    # a Lasso range prove under both kinds of profiling (the launch events, the live events; the helper ctx, its worker and
    # the stage events of the precommit), and the verifier
    n, table = 10, hl.LassoTable.range(2, 8)
    ss10 = [rng.randrange(1, P) for _ in range(10)]
    pp10, vp10 = hl.MultilinearKzg.setup(ctx, ss10), hl.MultilinearKzgVerifierParams.setup(ss10)
    dims = [ctx.upload(array.array("I", [rng.randrange(1 << 8) for _ in range(1 << n)]).tobytes()) for _ in range(2)]
    proofs = []
    for mode in (1, 2):
        hl.profile_enable(ctx, mode)
        t = hl.Keccak256Transcript()
        hl.lasso_prove(pp10, table, n, dims, t)
        proofs.append(t.into_proof())
        assert hl.profile_read(ctx)
    hl.profile_enable(ctx, 0)
    assert proofs[0] == proofs[1]
    hl.lasso_verify(vp10, table, n, hl.Keccak256Transcript.from_proof(proofs[0]))

    # a HyperPlonk vanilla prove of 2^6 rows, against the oracle
    o_pp, instances, o_proof, g_proof = thp._prove_both(hl, ctx, 6, False, 52)
    assert g_proof == o_proof

    # one param of every scheme
    pp6 = hl.MultilinearKzg.setup(ctx, SS)
    usrs = hl.Zeromorph.setup(ctx, 7, 64)
    assert len(usrs.powers()) == 64
    ipa = hl.Ipa.setup(ctx, 64)
    assert ipa.download() == hl.Ipa.setup(None, 64).download()
    bd = hl.Brakedown.setup(ctx, 6, 1, SEED)
    polys = _polys(hl, ctx, rng, 3, 6)
    comms = hl.Brakedown.batch_commit(bd, polys)
    assert [c.root for c in comms] == [hl.Brakedown.commit(bd, p).root for p in polys]  # (the single commits go with the expression)
    assert len(comms[1].staged(bd)) == 32 * bd.num_rows * bd.codeword_len

    # a Spark polynomial and an R1CS key: the golden commitments
    dims_m, val_m = spr.case_entries("matrix")
    assert spr.CASES["matrix"] == (5, 3, 2)
    cols = [hl.U32Column(ctx.upload(array.array("I", d).tobytes()), 5) for d in dims_m]
    poly = hl.spark_commit(ctx, pp6, cols, hl.MultilinearPolynomial.new(ctx, val_m), 3)
    golden = json.load(open(os.path.join(HERE, "golden", "spark.json")))["cases"]["matrix"]
    assert poly.commitment.hex() == golden["commitment"]
    small = min(spa.CASES, key=lambda k: spa.CASES[k])
    nk, lk, _ = spa.CASES[small]
    up = lambda col: hl.U32Column(ctx.upload(array.array("I", col).tobytes()), nk)
    inst = spa.case_instance(small)[0]
    key = hl.r1cs_commit(ctx, pp6, [(up(row), up(col), hl.MultilinearPolynomial.new(ctx, val)) for row, col, val in inst], lk)
    gk = json.load(open(os.path.join(HERE, "golden", "spartan.json")))["cases"][small]
    assert (len(key.commitment), hashlib.sha256(key.commitment).hexdigest()) == (gk["key_bytes"], gk["key_sha256"])

    # half of the handles by hand; the Spark polynomial and the key are left to the ctx; one commitment of the batch goes
    # before the others, one after the ctx
    assert _live(lib) != before
    pp10.free(), pp6.free(), ipa.free()
    comms[0].free()
    gc.collect()  # (the HyperPlonk param's SRS, while its ctx is there to free it)
    ctx.close()
    comms[1].free(), comms[2].free()
    bd.free()
    lib.lh_usrs_free(None, usrs.h)
    usrs.h = None
    assert _live(lib) == before


# ------------------------------------------------------------------ 2. the caller's device stays current
_ON_DEVICE_ONE = r"""
import random, sys, torch
sys.path.insert(0, sys.argv[1])
import halo2_lasso_amd as hl
assert torch.cuda.device_count() >= 2
torch.cuda.set_device(0)
here = torch.cuda.current_device
ctx = hl.Context(1)
torch.cuda.set_device(0)
bd = hl.Brakedown.setup(ctx, 6, 1, bytes(range(32)))
assert here() == 0, "setup"
rng = random.Random(62)
comm = hl.Brakedown.commit(bd, hl.MultilinearPolynomial.new(ctx, [rng.randrange(hl.R_MOD) for _ in range(64)]))
assert here() == 0, "commit"
comm.free()
assert here() == 0, "commitment freed"
bd.free()
assert here() == 0, "param freed"
ctx.close()
assert here() == 0, "ctx destroyed"
print("device 0 stayed current")
"""


def test_freeing_on_another_device_leaves_the_current_one(hl):
    """Where there are two devices (torch.cuda.device_count() >= 2): with device 0 current, a ctx, a Brakedown param and a
    commitment on device 1 are made, freed and destroyed, and hipGetDevice - through torch - still says 0 after each call.
    In a process of its own: a process in which torch has counted the devices does not bring up RCCL afterwards
    (ncclCommInitRank: no ROCm-capable device), which tests/test_gpu_sharded.py does further on in this one."""
    import subprocess
    import sys
    try:
        hl.Context(1).close()
    except hl.DeviceError:
        pytest.skip("needs two devices (torch.cuda.device_count() >= 2)")
    hl.Context(0).close()  # (creating a ctx leaves its device current: this process goes on on device 0)
    r = subprocess.run([sys.executable, "-c", _ON_DEVICE_ONE, os.path.dirname(HERE)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "device 0 stayed current" in r.stdout, r.stdout + r.stderr


# ------------------------------------------------------------------ 3. a creation entry that fails half-way
def _fails_cleanly_then_works(hl, lib, make, result, free):
    """make() under a failure of its 1st, 2nd, ... acquisition: DeviceError and the counts of before, until it goes through -
    with the result of the call nobody disturbed (made first: a ctx's lazy state exists from then on)"""
    first = make()
    want = result(first)
    free(first)
    for n in range(66):
        before = _live(lib)
        assert lib.lh_debug_fail_acquire_after(n) == 0
        try:
            got = make()
        except hl.DeviceError:
            assert _live(lib) == before, "acquisition %d failed and something stayed behind" % n
            continue
        finally:
            assert lib.lh_debug_fail_acquire_after(-1) == 0
        break
    # every one of these entries acquires something (the hook fired), and none acquires more than 64 things
    assert 1 <= n <= 64
    assert result(got) == want
    free(got)


def test_creation_entries_that_fail_hold_nothing(hl):
    from halo2_lasso_amd import _ffi
    lib = _ffi.load()
    rng = random.Random(63)
    check = lambda make, result, free=lambda h: h.free(): _fails_cleanly_then_works(hl, lib, make, result, free)
    check(lambda: hl.Context(0), lambda c: c.compute_units(), lambda c: c.close())
    ctx = hl.Context(0)
    srs3 = hl.MultilinearKzg.setup(ctx, SS[:3])
    flat = srs3.eqs_bytes()
    check(lambda: hl.MultilinearKzg.upload_bytes(ctx, flat, 3), lambda pp: pp.eqs_bytes())
    powers = hl.Zeromorph.setup(ctx, 7, 8).powers()
    check(lambda: hl.Zeromorph.upload(ctx, powers), lambda u: u.powers())
    check(lambda: hl.Ipa.setup(ctx, 8), lambda p: p.download())
    poly = _polys(hl, ctx, rng, 1, 6)[0]
    root = lambda bd: hl.Brakedown.commit(bd, poly).root
    check(lambda: hl.Brakedown.setup(ctx, 6, 1, SEED), lambda bd: (bd.info(), root(bd)))
    bd = hl.Brakedown.setup(ctx, 6, 1, SEED)
    check(lambda: hl.Brakedown.commit(bd, poly), lambda c: (c.root, c.rows(bd.num_rows, bd.codeword_len)))
    bd.free(), srs3.free()
    ctx.close()
