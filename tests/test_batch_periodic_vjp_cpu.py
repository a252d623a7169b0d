"""CPU tests of the periodic parameter-gradient boundary (cf_compute_batch_periodic_vjp and its host
form, include/chargeflux.h): the symbols exist and reject a null handle without touching a device
or the gradient array, the API version is unchanged (the addition is additive), and the Python
wrappers check the boxes' shape, dtype, contiguity and count before the C call."""
import ctypes as C

import numpy as np
import pytest

from openmmcoul import HipCalcCoulForceKernel, _cabi

N = 6
BOX = np.diag([1.0, 1.1, 1.2])


def test_symbols_are_exported_and_reject_a_null_handle():
    lib = _cabi.load_library()
    pos = np.zeros((2, N, 3))
    boxes = np.ascontiguousarray(np.broadcast_to(BOX, (2, 3, 3)))
    grad = np.full((2, N), 5.0)
    p = pos.ctypes.data_as(C.POINTER(C.c_double))
    b = boxes.ctypes.data_as(C.POINTER(C.c_double))
    g = grad.ctypes.data_as(C.POINTER(C.c_double))
    assert hasattr(lib, "cf_compute_batch_periodic_vjp") and hasattr(lib, "cf_compute_batch_periodic_vjp_host")
    assert lib.cf_compute_batch_periodic_vjp(None, 2, C.c_void_p(pos.ctypes.data), b, None, None, None,
                                             C.c_void_p(grad.ctypes.data)) == _cabi.CF_ERR_INVALID
    assert b"null" in lib.cf_last_error()
    assert lib.cf_compute_batch_periodic_vjp_host(None, 2, p, b, None, None, None, g) == _cabi.CF_ERR_INVALID
    assert b"null" in lib.cf_last_error()
    assert (grad == 5.0).all()


def test_api_version_is_still_4():
    assert _cabi.load_library().cf_api_version() == 4


def _uninitialised_kernel():
    # no device here: the wrappers must raise before they reach the (null) handle
    k = HipCalcCoulForceKernel()
    k._n = N
    return k


BAD_BOXES = [
    np.zeros((2, 3, 2)),                                   # wrong trailing shape
    np.zeros((2, 9)),                                      # flat boxes
    np.zeros(9),
    np.zeros((3, 3, 3)),                                   # 3 boxes for 2 conformations
    np.zeros((1, 3, 3)),                                   # no implicit broadcast of (1, 3, 3)
    np.zeros((2, 3, 3), dtype=np.float32),                 # wrong dtype
    np.zeros((3, 3), dtype=np.float32),
    np.zeros((2, 3, 3)).transpose(0, 2, 1),                # right shape, not C-contiguous
    [[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]],               # not a numpy array
]


@pytest.mark.parametrize("boxes", BAD_BOXES, ids=range(len(BAD_BOXES)))
def test_host_wrapper_rejects_bad_boxes(boxes):
    k = _uninitialised_kernel()
    with pytest.raises(ValueError):
        k.execute_batch_vjp_host(np.zeros((2, N, 3)), energy_bar=np.ones(2), boxes=boxes)


@pytest.mark.parametrize("boxes", BAD_BOXES, ids=range(len(BAD_BOXES)))
def test_device_wrapper_rejects_bad_boxes(boxes):
    import torch
    k = _uninitialised_kernel()
    f64 = torch.float64
    with pytest.raises(ValueError):
        k.execute_batch_vjp_device(torch.zeros((2, N, 3), dtype=f64), torch.zeros((2, N), dtype=f64),
                                   energy_bar=torch.ones(2, dtype=f64), boxes=boxes)


def test_a_torch_tensor_is_not_a_box_array():
    # the boxes are host numpy memory for the device form too
    import torch
    k = _uninitialised_kernel()
    f64 = torch.float64
    tb = torch.zeros((2, 3, 3), dtype=f64)
    with pytest.raises(ValueError):
        k.execute_batch_vjp_host(np.zeros((2, N, 3)), boxes=tb)
    with pytest.raises(ValueError):
        k.execute_batch_vjp_device(torch.zeros((2, N, 3), dtype=f64), torch.zeros((2, N), dtype=f64), boxes=tb)


def test_wrappers_still_check_positions_and_cotangents_first():
    import torch
    k = _uninitialised_kernel()
    with pytest.raises(ValueError):
        k.execute_batch_vjp_host(np.zeros((2, N + 1, 3)), boxes=BOX)
    with pytest.raises(ValueError):
        k.execute_batch_vjp_host(np.zeros((2, N, 3)), charges_bar=np.zeros((3, N)), boxes=BOX)
    with pytest.raises(ValueError):
        k.execute_batch_vjp_device(torch.zeros((2, N, 3), dtype=torch.float32),
                                   torch.zeros((2, N), dtype=torch.float64), boxes=BOX)


def test_fitting_layer_rejects_bad_boxes_before_loading_parameters():
    import torch
    from openmmcoul.fitting import BatchedChargeFlux

    model = BatchedChargeFlux(_uninitialised_kernel(), None)   # neither is reached
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64)
    with pytest.raises(ValueError):
        model(z(N), z(0, 2), z(0, 2), z(0, 5), z(2, N, 3), boxes=np.zeros((3, 3, 3)))
    with pytest.raises(ValueError):
        model(z(N), z(0, 2), z(0, 2), z(0, 5), z(2, N, 3), boxes=z(2, 3, 3))
    assert model._loads == 0
