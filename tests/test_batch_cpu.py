"""CPU tests of the batched-evaluation boundary (cf_compute_batch and friends, include/chargeflux.h):
the symbols exist and reject null handles without touching a device, the Python wrappers check
shapes and dtypes before the C call, and the API version is unchanged (the addition is additive)."""
import ctypes as C

import numpy as np
import pytest

from openmmcoul import HipCalcCoulForceKernel, _cabi

N = 6


def test_null_handles_are_rejected():
    lib = _cabi.load_library()
    pos = np.zeros((2, N, 3))
    p = pos.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.cf_compute_batch(None, 2, C.c_void_p(pos.ctypes.data), 3, None, None, None) == _cabi.CF_ERR_INVALID
    assert b"null" in lib.cf_last_error()
    assert lib.cf_compute_batch_host(None, 2, p, 3, None, None, None) == _cabi.CF_ERR_INVALID
    a = C.c_int64(7)
    assert lib.cf_get_batch_stats(None, C.byref(a), None, None) == _cabi.CF_ERR_INVALID
    assert a.value == 7
    assert lib.cf_set_batch_limit(None, 1) == _cabi.CF_ERR_INVALID


def test_api_version_is_still_4():
    assert _cabi.load_library().cf_api_version() == 4


def _uninitialised_kernel():
    # no device here: the wrappers must raise before they reach the (null) handle
    k = HipCalcCoulForceKernel()
    k._n = N
    return k


def test_host_wrapper_rejects_bad_shape_and_dtype():
    k = _uninitialised_kernel()
    with pytest.raises(ValueError):
        k.execute_batch_host(np.zeros((2, N + 1, 3)))
    with pytest.raises(ValueError):
        k.execute_batch_host(np.zeros((2, N, 3), dtype=np.float32))
    with pytest.raises(ValueError):
        k.execute_batch_host(np.zeros((N, 3)))
    with pytest.raises(ValueError):
        k.execute_batch_host(np.zeros((2, 3, N)).transpose(0, 2, 1))   # right shape, not C-contiguous
    with pytest.raises(ValueError):
        k.execute_batch_host(np.zeros((2, N, 3)), forces=np.zeros((3, N, 3)))


def test_device_wrapper_rejects_bad_shape_and_dtype():
    import torch
    k = _uninitialised_kernel()
    with pytest.raises(ValueError):
        k.execute_batch_device(torch.zeros((2, N + 1, 3), dtype=torch.float64), True, True)
    with pytest.raises(ValueError):
        k.execute_batch_device(torch.zeros((2, N, 3), dtype=torch.float32), True, True)
    with pytest.raises(ValueError):
        k.execute_batch_device(torch.zeros((2, N, 3), dtype=torch.float64), True, True,
                               energies=torch.zeros(3, dtype=torch.float64))
    with pytest.raises(ValueError):
        k.execute_batch_device(np.zeros((2, N, 3)), True, True)
