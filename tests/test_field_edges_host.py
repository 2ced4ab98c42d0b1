"""The host forms of the field and curve primitives (ff.cuh's generic path, ec.cuh's LH_HD formulas) on the same edge
tables as tests/test_gpu_field_edges.py, through the probe's host entry: no GPU needed.  mul_scan and the two dot forms
run as the host's mul / dot; Wide, add_mixed_lazy and the quad routines are device-only and have no host form."""
import ctypes as C

import pytest

import field_edges as fe


@pytest.fixture(scope="module")
def run():
    return fe.Probe().runner(host=True)


@pytest.mark.parametrize("field", ["Fr", "Fq"])
@pytest.mark.parametrize("op", fe.FIELD_OPS)
def test_field_op_host(run, op, field):
    bad = fe.check_field_op(run, op, field)
    assert not bad, fe.report(bad)


@pytest.mark.parametrize("field", ["Fr", "Fq"])
@pytest.mark.parametrize("k", fe.DOT_KS)
def test_dot_host(run, k, field):
    bad = fe.check_dot(run, "dot_cols", field, k)
    assert not bad, fe.report(bad)


@pytest.mark.parametrize("field", ["Fr", "Fq"])
def test_dot2_lazy_operands_host(run, field):
    bad = fe.check_dot(run, "dot_cols", field, 2, lazy=True)
    assert not bad, fe.report(bad)


@pytest.mark.parametrize("op", [op for op in fe.CURVE_OPS if op not in fe.DEVICE_ONLY])
def test_curve_host(run, op):
    bad = fe.check_curve(run, op)
    assert not bad, fe.report(bad)


@pytest.mark.parametrize("op", sorted(fe.DEVICE_ONLY))
def test_device_only_ops_are_refused_on_the_host(op):
    """the host entry answers -9 for an op without a host form instead of running something else"""
    lib = fe.Probe().lib
    field = 0 if op == "wide" else 1
    stride = 128
    buf = (C.c_uint32 * stride)()
    out = (C.c_uint32 * 128)()
    assert lib.ffp_run_host(fe.OP_ID[op], field, 0, C.addressof(buf), stride, C.addressof(out), 128, 1) == -9
