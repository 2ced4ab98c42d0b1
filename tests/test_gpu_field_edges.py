"""The device field and curve primitives (csrc/ff.cuh, wide.cuh, ec.cuh) at their carry and range edges, one probe
launch per op (csrc/ff_probe.hip), against the big-integer reference of tests/field_edges.py.

Values are checked exactly modulo p, canonical outputs below p, lazy outputs below 2 p; dot products of canonical
operands must be canonical for every band of the unreduced result up to the top one; Wide's raw limbs must equal the
exact sum; XYZZ results must satisfy ZZ^3 = ZZZ^2 and have the affine value of oracle.pyref.curve, and the four lanes of
the quad routines must agree."""
import pytest

import field_edges as fe

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def run():
    return fe.Probe().runner(host=False)


@pytest.mark.parametrize("field", ["Fr", "Fq"])
@pytest.mark.parametrize("op", fe.FIELD_OPS)
def test_field_op(run, op, field):
    bad = fe.check_field_op(run, op, field)
    assert not bad, fe.report(bad)


@pytest.mark.parametrize("field", ["Fr", "Fq"])
@pytest.mark.parametrize("k", fe.DOT_KS)
@pytest.mark.parametrize("form", ["dot_scan", "dot_cols"])
def test_dot(run, form, k, field):
    bad = fe.check_dot(run, form, field, k)
    assert not bad, fe.report(bad)


@pytest.mark.parametrize("field", ["Fr", "Fq"])
@pytest.mark.parametrize("form", ["dot_scan", "dot_cols"])
def test_dot2_lazy_operands(run, form, field):
    """dot<2> as add_mixed_lazy uses it: operands in [0, 2 p), result below 2 p"""
    bad = fe.check_dot(run, form, field, 2, lazy=True)
    assert not bad, fe.report(bad)


def test_wide(run):
    bad = fe.check_wide(run)
    assert not bad, fe.report(bad)


@pytest.mark.parametrize("op", fe.CURVE_OPS)
def test_curve(run, op):
    bad = fe.check_curve(run, op)
    assert not bad, fe.report(bad)
