"""CPU: what of the Hyrax row commitments (csrc/kernels_hyrax.hip) exists without a device: the C entry lh_g1_rows_msm is
exported with the eight arguments the binding passes and refuses a null ctx before anything touches a device, and the Python
side has Hyrax.rows_msm.  What the kernels compute is tests/test_gpu_hyrax_rows.py; the option hyrax_rows is exercised by
tests/test_gpu_hyrax_provers.py."""
import inspect

import halo2_lasso_amd as hl
from halo2_lasso_amd import _ffi


def test_the_entry_is_exported():
    lib = _ffi.load()
    assert hasattr(lib, "lh_g1_rows_msm") and len(lib.lh_g1_rows_msm.argtypes) == 8


def test_null_ctx_is_an_argument_error_before_anything_touches_a_device():
    lib = _ffi.load()
    assert lib.lh_g1_rows_msm(None, None, 0, 0, 0, 1, None, None) == _ffi.LH_ERR_ARG
    assert b"null argument" in lib.lh_last_error()


def test_python_surface():
    assert list(inspect.signature(hl.Hyrax.rows_msm).parameters) == ["ctx", "scalars_buf", "n", "row_len", "bases_buf", "u32", "bits"]
