"""CPU tests of the parameter-gradient boundary (cf_get_param_counts, cf_compute_batch_vjp,
cf_compute_batch_vjp_host; include/chargeflux.h): the symbols exist and reject null handles without
touching a device, the API version is unchanged (the addition is additive), and the Python wrappers
check shape, dtype and contiguity before the C call."""
import ctypes as C

import numpy as np
import pytest

from openmmcoul import HipCalcCoulForceKernel, _cabi

N = 6


def test_null_handles_are_rejected():
    lib = _cabi.load_library()
    pos = np.zeros((2, N, 3))
    grad = np.full((2, N), 5.0)
    p = pos.ctypes.data_as(C.POINTER(C.c_double))
    g = grad.ctypes.data_as(C.POINTER(C.c_double))
    counts = (C.c_int32 * 4)(7, 7, 7, 7)
    assert lib.cf_get_param_counts(None, counts) == _cabi.CF_ERR_INVALID
    assert b"null" in lib.cf_last_error()
    assert list(counts) == [7, 7, 7, 7]
    assert lib.cf_compute_batch_vjp(None, 2, C.c_void_p(pos.ctypes.data), None, None, None,
                                    C.c_void_p(grad.ctypes.data)) == _cabi.CF_ERR_INVALID
    assert b"null" in lib.cf_last_error()
    assert lib.cf_compute_batch_vjp_host(None, 2, p, None, None, None, g) == _cabi.CF_ERR_INVALID
    assert b"null" in lib.cf_last_error()
    assert (grad == 5.0).all()


def test_api_version_is_still_4():
    assert _cabi.load_library().cf_api_version() == 4


def _uninitialised_kernel():
    # no device here: the wrappers must raise before they reach the (null) handle
    k = HipCalcCoulForceKernel()
    k._n = N
    return k


def test_host_wrapper_rejects_bad_arrays():
    k = _uninitialised_kernel()
    pos = np.zeros((2, N, 3))
    with pytest.raises(ValueError):
        k.execute_batch_vjp_host(np.zeros((2, N + 1, 3)))
    with pytest.raises(ValueError):
        k.execute_batch_vjp_host(np.zeros((2, N, 3), dtype=np.float32))
    with pytest.raises(ValueError):
        k.execute_batch_vjp_host(np.zeros((N, 3)))
    with pytest.raises(ValueError):
        k.execute_batch_vjp_host(np.zeros((2, 3, N)).transpose(0, 2, 1))   # right shape, not C-contiguous
    with pytest.raises(ValueError):
        k.execute_batch_vjp_host(pos.tolist())
    # cotangents: another B, wrong trailing shape, dtype, contiguity
    with pytest.raises(ValueError):
        k.execute_batch_vjp_host(pos, energy_bar=np.zeros(3))
    with pytest.raises(ValueError):
        k.execute_batch_vjp_host(pos, charges_bar=np.zeros((3, N)))
    with pytest.raises(ValueError):
        k.execute_batch_vjp_host(pos, forces_bar=np.zeros((3, N, 3)))
    with pytest.raises(ValueError):
        k.execute_batch_vjp_host(pos, charges_bar=np.zeros((2, N + 1)))
    with pytest.raises(ValueError):
        k.execute_batch_vjp_host(pos, energy_bar=np.zeros(2, dtype=np.float32))
    with pytest.raises(ValueError):
        k.execute_batch_vjp_host(pos, forces_bar=np.zeros((2, 3, N)).transpose(0, 2, 1))
    with pytest.raises(ValueError):
        k.execute_batch_vjp_host(pos, charges_bar=np.zeros((2, 2 * N))[:, ::2])


def test_device_wrapper_rejects_bad_arrays():
    import torch
    k = _uninitialised_kernel()
    f64 = torch.float64
    pos = torch.zeros((2, N, 3), dtype=f64)
    grad = torch.zeros((2, N), dtype=f64)
    with pytest.raises(ValueError):
        k.execute_batch_vjp_device(torch.zeros((2, N + 1, 3), dtype=f64), grad)
    with pytest.raises(ValueError):
        k.execute_batch_vjp_device(torch.zeros((2, N, 3), dtype=torch.float32), grad)
    with pytest.raises(ValueError):
        k.execute_batch_vjp_device(torch.zeros((2, 3, N), dtype=f64).transpose(1, 2), grad)
    with pytest.raises(ValueError):
        k.execute_batch_vjp_device(np.zeros((2, N, 3)), grad)
    with pytest.raises(ValueError):
        k.execute_batch_vjp_device(pos, grad, energy_bar=torch.zeros(3, dtype=f64))
    with pytest.raises(ValueError):
        k.execute_batch_vjp_device(pos, grad, charges_bar=torch.zeros((3, N), dtype=f64))
    with pytest.raises(ValueError):
        k.execute_batch_vjp_device(pos, grad, forces_bar=torch.zeros((3, N, 3), dtype=f64))
    with pytest.raises(ValueError):
        k.execute_batch_vjp_device(pos, grad, forces_bar=torch.zeros((2, N, 3), dtype=torch.float32))
    with pytest.raises(ValueError):
        k.execute_batch_vjp_device(pos, grad, charges_bar=torch.zeros((2, 2 * N), dtype=f64)[:, ::2])
    with pytest.raises(ValueError):
        k.execute_batch_vjp_device(pos, grad, energy_bar=np.zeros(2))
    with pytest.raises(ValueError):
        k.execute_batch_vjp_device(pos, grad.numpy())
