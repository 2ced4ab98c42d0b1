"""CPU tests of the boundary: the in-tree library loads, exports every symbol include/lasso_hip.h
declares, the ctypes mirrors of the ABI structs have the C sizes, and compute fails loudly without a GPU."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "lasso_hip.h")).read()


def declared_symbols():
    return sorted(set(re.findall(r"\b(lh_[a-z0-9_]+)\s*\(", HEADER)))


def test_library_exports_every_declared_symbol(hl):
    from halo2_lasso_amd import _ffi
    lib = _ffi.load()
    syms = declared_symbols()
    assert len(syms) >= 40
    for name in syms:
        assert hasattr(lib, name), "liblasso_hip.so does not export %s" % name
    assert set(_ffi.SIGNATURES) == set(syms), "ctypes binding and header disagree"


def test_struct_layouts(hl):
    from halo2_lasso_amd import _ffi
    assert C.sizeof(_ffi.lh_fr) == 32 and C.sizeof(_ffi.lh_g1) == 64
    assert C.sizeof(_ffi.lh_evaluation) == 40
    assert C.sizeof(_ffi.lh_sop) == 8 + 32 * 48 + 48 + 48 * 4
    assert C.sizeof(_ffi.lh_lasso_table) == 12 + 64 + 64 + 4 + 32 * 16 + 16 + 16 * 4 + 0 \
        or C.sizeof(_ffi.lh_lasso_table) % 8 == 0
    assert C.sizeof(_ffi.lh_transcript) == 8 * C.sizeof(C.c_void_p)
    assert C.sizeof(_ffi.lh_g2) == 128
    assert C.sizeof(_ffi.lh_debug_u32_args) == 9 * 8 + 2 * 32 + 3 * 8 and _ffi.lh_debug_u32_args.r0.offset == 72


def test_marshalling(hl):
    for v in (0, 1, 2 ** 200 + 17, hl.R_MOD - 1):
        assert hl.fr_from_bytes(hl.fr_to_bytes(v)) == v
    # Montgomery form of 1 is R mod r
    assert hl.fr_to_bytes(1) == bytes.fromhex("fbffff4f1c3496ac29cd609f9576fc362e4679786fa36e662fdf079ac1770a0e")
    assert hl.g1_from_bytes(hl.g1_to_bytes((1, 2))) == (1, 2)
    assert hl.g1_from_bytes(hl.g1_to_bytes(None)) is None
    t = hl.LassoTable.range(2, 16).to_c()
    assert (t.num_chunks, t.chunk_bits, t.num_memories, t.num_terms) == (2, 16, 2, 2)
    assert hl.fr_from_bytes(bytes(t.g_coeff[1])) == 1 << 16


def test_keccak_transcript_host_side(hl):
    """The built-in transcript is host code: usable (and checkable against the oracle) without a GPU."""
    from oracle.pyref.transcript import Keccak256Transcript as OT
    t, ot = hl.Keccak256Transcript(), OT()
    for v in (0, 1, hl.R_MOD - 1, 1 << 255):
        t.write_field_element(v), ot.write_field_element(v)
        assert t.squeeze_challenge() == ot.squeeze_challenge()
    t.common_field_element(7), ot.common_field_element(7)
    t.write_commitment((1, 2)), ot.write_commitment((1, 2))
    assert t.squeeze_challenges(3) == ot.squeeze_challenges(3)
    assert t.into_proof() == ot.into_proof()
    with pytest.raises(hl.TranscriptError):
        t.write_commitment(None)


def test_no_gpu_means_loud_failure(hl):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(hl.DeviceError):
        hl.Context(0)


def _live(lib):
    """lh_debug_live_resources: (device blocks, pinned blocks, events, streams) the library's owners hold right now"""
    out = (C.c_uint64 * 4)()
    assert lib.lh_debug_live_resources(out) == 0
    return tuple(out)


def test_a_failed_context_holds_nothing(hl):
    """without a GPU Context(0) fails and the process holds nothing at all; beside one, a device that does not exist"""
    from halo2_lasso_amd import _ffi
    lib = _ffi.load()
    assert lib.lh_debug_live_resources(None) == _ffi.LH_ERR_ARG
    before = _live(lib)
    try:
        hl.Context(0).close()
    except hl.DeviceError:
        assert _live(lib) == before == (0, 0, 0, 0)
        return
    with pytest.raises(hl.DeviceError):
        hl.Context(1 << 20)
    assert _live(lib) == before


def test_host_only_handles_hold_no_device_resource(hl):
    """handles made without a ctx come and go with the counts unchanged (a failure injected into the owners never meets them)"""
    from halo2_lasso_amd import _ffi
    lib = _ffi.load()
    before = _live(lib)
    assert lib.lh_debug_fail_acquire_after(0) == 0
    try:
        made = [hl.BrakedownVerifierParam.derive(6, 1), hl.BrakedownVerifierParam.setup(4, 1, bytes(range(32))),
                hl.MultilinearKzgVerifierParams.setup([3, 5]), hl.ZeromorphVerifierParam.setup(7, 8, 8),
                hl.UnivariateKzgVerifierParam.setup(7), hl.Ipa.setup(None, 8)]
        assert _live(lib) == before
        for h in made:
            h.free()
        assert _live(lib) == before
    finally:
        assert lib.lh_debug_fail_acquire_after(-1) == 0


def test_cpu_list_format(hl):
    """the kernel's CPU list format of sysfs local_cpulist, as Context.host_cpus reads it"""
    assert hl.parse_cpulist("0-3,8,10-11\n") == {0, 1, 2, 3, 8, 10, 11}
    assert hl.parse_cpulist("") == set() and hl.parse_cpulist("5") == {5}
    assert len(hl.parse_cpulist("0-63,128-191")) == 128


@pytest.mark.gpu
def test_host_binding_next_to_the_device(hl, ctx):
    """lh_ctx_host_cpus names the device's PCI address and the CPUs on its NUMA node; Context.bind_host narrows the calling
    thread's affinity to them (never widens it, never leaves it empty) and hands back what it replaced."""
    bus, local = ctx.host_cpus()
    assert re.fullmatch(r"[0-9a-f]{4}:[0-9a-f]{2}:[0-9a-f]{2}\.[0-9a-f]", bus), bus
    assert os.path.isdir("/sys/bus/pci/devices/" + bus)
    before = os.sched_getaffinity(0)
    prev = ctx.bind_host()
    try:
        now = os.sched_getaffinity(0)
        if prev is None:
            assert now == before and (not (local & before) or (local & before) == before)
        else:
            assert prev == before and now == (local & before) and now and now < before
    finally:
        os.sched_setaffinity(0, before)


@pytest.mark.gpu
def test_null_arguments_are_errors_not_crashes(hl, ctx):
    """Every pointer an entry point dereferences is checked at the boundary (capi.cpp NEED / NEED_N): NULL is LH_ERR_ARG with
    a message naming the argument, never a segfault inside the library; an empty vector may be NULL."""
    from halo2_lasso_amd import _ffi
    lib, h = ctx.lib, ctx.h
    pp = hl.MultilinearKzg.setup(ctx, [3, 5, 7])
    poly = ctx.upload(b"".join(hl.fr_to_bytes(v) for v in range(8)))
    out, fr = _ffi.lh_g1(), _ffi.lh_fr()
    tr = hl.Keccak256Transcript()
    bad = [
        lib.lh_mkzg_commit(h, pp.h, None, 3, C.byref(out)),
        lib.lh_mkzg_commit(h, pp.h, poly.ptr, 3, None),
        lib.lh_mkzg_commit(h, None, poly.ptr, 3, C.byref(out)),
        lib.lh_mkzg_batch_commit(h, pp.h, None, 1, 3, C.byref(out)),
        lib.lh_mkzg_batch_commit(h, pp.h, (C.c_void_p * 1)(poly.ptr), 1, 3, None),
        lib.lh_mkzg_open(h, pp.h, None, 3, (_ffi.lh_fr * 3)(), tr.p, C.byref(fr)),
        lib.lh_mkzg_open(h, pp.h, poly.ptr, 3, None, tr.p, C.byref(fr)),
        lib.lh_mkzg_open(h, pp.h, poly.ptr, 3, (_ffi.lh_fr * 3)(), None, C.byref(fr)),
        lib.lh_mkzg_batch_open(h, pp.h, 3, None, 1, (_ffi.lh_fr * 3)(), 1, (_ffi.lh_evaluation * 1)(), 1, tr.p),
        lib.lh_mkzg_batch_open(h, pp.h, 3, (C.c_void_p * 1)(poly.ptr), 1, None, 1, (_ffi.lh_evaluation * 1)(), 1, tr.p),
        lib.lh_mkzg_batch_open(h, pp.h, 3, (C.c_void_p * 1)(poly.ptr), 1, (_ffi.lh_fr * 3)(), 1, None, 1, tr.p),
        lib.lh_mkzg_setup(h, None, 3, C.byref(C.c_void_p())),
        lib.lh_srs_upload(h, None, 3, C.byref(C.c_void_p())),
        lib.lh_srs_download(h, pp.h, None),
        lib.lh_msm(h, None, None, 4, C.byref(out)),
        lib.lh_msm_u32(h, poly.ptr, None, 4, C.byref(out)),
        lib.lh_fr_add(h, poly.ptr, None, 8, poly.ptr),
        lib.lh_fr_batch_invert(h, None, 8, poly.ptr),
        lib.lh_fix_var(h, poly.ptr, 8, C.byref(fr), None),
        lib.lh_eq_xy(h, None, 3, poly.ptr),
        lib.lh_evaluate(h, None, 1, 3, (_ffi.lh_fr * 3)(), C.byref(fr)),
        lib.lh_lincomb(h, (C.c_void_p * 1)(poly.ptr), None, 1, 8, poly.ptr),
        lib.lh_upload(h, None, b"1234", 4),
        lib.lh_ctx_compute_units(h, None),
        lib.lh_download(h, None, poly.ptr, 4),
        lib.lh_zeromorph_open(h, None, 8, poly.ptr, 3, (_ffi.lh_fr * 3)(), tr.p),
        lib.lh_zeromorph_batch_commit(h, None, 8, (C.c_void_p * 1)(poly.ptr), 1, 3, C.byref(out)),
    ]
    assert bad == [_ffi.LH_ERR_ARG] * len(bad), bad
    assert b"null argument" in lib.lh_last_error() or b"transcript" in lib.lh_last_error()
    # the test-only entry of the 32-bit column kernels: every pointer of its argument block that an operation uses
    col, dst = ctx.upload(bytes(64)), ctx.alloc(4 * 32)
    taken, sums = C.c_int(0), (_ffi.lh_fr * 4)()
    full = dict(d_cols=(C.c_void_p * 1)(col.ptr), lens=(C.c_size_t * 1)(4), w=(_ffi.lh_fr * 1)(), count=1, d_weights=poly.ptr,
                n=1, d_fr=(C.c_void_p * 1)(poly.ptr), w_fr=(_ffi.lh_fr * 1)(), num_fr=1, d_out=dst.ptr, out_host=sums,
                taken=C.pointer(taken))
    used = {"d_cols": range(8), "lens": (3, 4, 5, 6), "w": (4, 5, 6), "d_weights": (0, 1, 2, 3, 6, 7), "d_fr": (4,), "w_fr": (4,),
            "d_out": (3, 4, 5, 6, 7), "out_host": (0, 1, 2, 6, 7), "taken": (5,)}
    bad = [lib.lh_debug_u32_columns(None, 0, C.byref(_ffi.lh_debug_u32_args(**full))), lib.lh_debug_u32_columns(h, 0, None)]
    for field, ops in used.items():
        for op in ops:
            bad.append(lib.lh_debug_u32_columns(h, op, C.byref(_ffi.lh_debug_u32_args(**{k: v for k, v in full.items() if k != field}))))
            assert b"null argument" in lib.lh_last_error(), (field, op, lib.lh_last_error())
    bad.append(lib.lh_debug_u32_columns(h, 0, C.byref(_ffi.lh_debug_u32_args(**dict(full, d_cols=(C.c_void_p * 1)(None))))))
    assert bad == [_ffi.LH_ERR_ARG] * len(bad), bad
    for op in range(8):  # ... and with everything in place each operation runs
        assert lib.lh_debug_u32_columns(h, op, C.byref(_ffi.lh_debug_u32_args(**full))) == _ffi.LH_OK, (op, lib.lh_last_error())
    # an empty vector may be NULL: nothing to read, nothing written
    assert lib.lh_mkzg_batch_commit(h, pp.h, None, 0, 3, None) == _ffi.LH_OK
    assert lib.lh_fr_add(h, None, None, 0, None) == _ffi.LH_OK
    assert lib.lh_upload(h, None, None, 0) == _ffi.LH_OK
    # ... and the ctx still proves after all of that
    assert hl.MultilinearKzg.commit(pp, hl.MultilinearPolynomial(ctx, poly, 3)) is not None


def _all_refused(lib, calls):
    """every call returns LH_ERR_ARG at the boundary, its message naming a null argument (or the transcript)"""
    from halo2_lasso_amd import _ffi
    for i, call in enumerate(calls):
        rc, msg = call(), lib.lh_last_error()
        assert rc == _ffi.LH_ERR_ARG and (b"null argument" in msg or b"transcript" in msg), (i, rc, msg)


def test_null_arguments_of_the_kzg_and_zeromorph_verifier_entry_points(hl):
    """lh_lasso_verify / lh_hyperplonk_verify[_phases] over multilinear KZG and Zeromorph: each pointer in turn NULL"""
    from halo2_lasso_amd import _ffi
    lib = _ffi.load()
    tbl, hvp, one = hl.LassoTable.range(2, 2).to_c(), _ffi.lh_hp_vparam(), (C.c_size_t * 1)(0)
    t = hl.Keccak256Transcript.from_proof(b"")
    for vp, suffix in ((hl.MultilinearKzgVerifierParams.setup([3, 5]), ""), (hl.ZeromorphVerifierParam.setup(7, 8, 8), "_zeromorph")):
        lasso, hp, hp_phases = (getattr(lib, name + suffix) for name in
                                ("lh_lasso_verify", "lh_hyperplonk_verify", "lh_hyperplonk_verify_phases"))
        _all_refused(lib, [
            lambda: lasso(None, C.byref(tbl), 2, t.p), lambda: lasso(vp.h, None, 2, t.p), lambda: lasso(vp.h, C.byref(tbl), 2, None),
            lambda: hp(None, C.byref(hvp), None, t.p), lambda: hp(vp.h, None, None, t.p), lambda: hp(vp.h, C.byref(hvp), None, None),
            lambda: hp_phases(None, C.byref(hvp), 1, one, one, None, t.p), lambda: hp_phases(vp.h, None, 1, one, one, None, t.p),
            lambda: hp_phases(vp.h, C.byref(hvp), 1, None, one, None, t.p), lambda: hp_phases(vp.h, C.byref(hvp), 1, one, None, None, t.p),
            lambda: hp_phases(vp.h, C.byref(hvp), 1, one, one, None, None)])


@pytest.mark.gpu
def test_null_arguments_of_the_kzg_and_zeromorph_prover_entry_points(hl, ctx):
    """lh_lasso_prove / lh_hyperplonk_prove[_phases] over multilinear KZG (the sharded entries too) and Zeromorph: each pointer
    in turn NULL returns at the boundary - nothing is proven - and the ctx still works"""
    from halo2_lasso_amd import _ffi
    lib, h = ctx.lib, ctx.h
    srs, usrs = hl.MultilinearKzg.setup(ctx, [3, 5]), hl.Zeromorph.setup(ctx, 7, 8)
    poly = ctx.upload(b"".join(hl.fr_to_bytes(v) for v in range(4)))
    tbl, ptrs, one, tr = hl.LassoTable.range(2, 2).to_c(), (C.c_void_p * 1)(poly.ptr), (C.c_size_t * 1)(0), hl.Keccak256Transcript()
    prm, prm1, circ = _ffi.lh_hp_param(), _ffi.lh_hp_param(), _ffi.lh_hp_circuit()
    prm1.num_witness_polys = 1
    circ.user, circ.synthesize = None, _ffi._SYNTH_CB(lambda *args: 0)
    for head, suffix in (((srs.h,), ""), ((usrs.h, 8), "_zeromorph")):
        none = (None,) + head[1:]
        lasso, hp, hp_phases = (getattr(lib, name + suffix) for name in
                                ("lh_lasso_prove", "lh_hyperplonk_prove", "lh_hyperplonk_prove_phases"))
        _all_refused(lib, [
            lambda: lasso(None, *head, C.byref(tbl), 2, ptrs, tr.p), lambda: lasso(h, *none, C.byref(tbl), 2, ptrs, tr.p),
            lambda: lasso(h, *head, None, 2, ptrs, tr.p), lambda: lasso(h, *head, C.byref(tbl), 2, None, tr.p),
            lambda: lasso(h, *head, C.byref(tbl), 2, ptrs, None),
            lambda: hp(None, *head, C.byref(prm), None, None, tr.p), lambda: hp(h, *none, C.byref(prm), None, None, tr.p),
            lambda: hp(h, *head, None, None, None, tr.p), lambda: hp(h, *head, C.byref(prm1), None, None, tr.p),
            lambda: hp(h, *head, C.byref(prm), None, None, None),
            lambda: hp_phases(None, *head, C.byref(prm), 1, one, one, None, C.byref(circ), tr.p),
            lambda: hp_phases(h, *none, C.byref(prm), 1, one, one, None, C.byref(circ), tr.p),
            lambda: hp_phases(h, *head, None, 1, one, one, None, C.byref(circ), tr.p),
            lambda: hp_phases(h, *head, C.byref(prm), 1, one, one, None, None, tr.p),
            lambda: hp_phases(h, *head, C.byref(prm), 1, None, one, None, C.byref(circ), tr.p),
            lambda: hp_phases(h, *head, C.byref(prm), 1, one, None, None, C.byref(circ), tr.p),
            lambda: hp_phases(h, *head, C.byref(prm), 1, one, one, None, C.byref(circ), None)])
    _all_refused(lib, [
        lambda: lib.lh_lasso_prove_sharded(None, srs.h, C.byref(tbl), 2, ptrs, tr.p),
        lambda: lib.lh_lasso_prove_sharded(h, None, C.byref(tbl), 2, ptrs, tr.p),
        lambda: lib.lh_lasso_prove_sharded(h, srs.h, None, 2, ptrs, tr.p),
        lambda: lib.lh_lasso_prove_sharded(h, srs.h, C.byref(tbl), 2, None, tr.p),
        lambda: lib.lh_lasso_prove_sharded(h, srs.h, C.byref(tbl), 2, ptrs, None),
        lambda: lib.lh_hyperplonk_prove_sharded(None, srs.h, C.byref(prm), None, None, tr.p),
        lambda: lib.lh_hyperplonk_prove_sharded(h, None, C.byref(prm), None, None, tr.p),
        lambda: lib.lh_hyperplonk_prove_sharded(h, srs.h, None, None, None, tr.p),
        lambda: lib.lh_hyperplonk_prove_sharded(h, srs.h, C.byref(prm1), None, None, tr.p)])
    assert tr.into_proof() == b""
    assert hl.MultilinearKzg.commit(srs, hl.MultilinearPolynomial(ctx, poly, 2)) is not None
