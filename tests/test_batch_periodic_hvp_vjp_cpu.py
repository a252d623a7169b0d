"""CPU tests of the boundary of cf_compute_batch_periodic_hvp_vjp (include/chargeflux.h): the two symbols
exist and reject a null handle without touching a device, and the wrappers' argument checks raise
before any device call.  They also guard the yardstick of the GPU tests
(tests/pbc_hvp_vjp_reference.py) on `w22`, one conformation and one direction: the central differences
at STEP and 2 STEP agree to the bound of tests/test_batch_hvp_vjp_cpu.py, a tenth of the GPU bar per
parameter group (max|a - b| <= 1e-10 max|a| + 1e-10).
"""
import ctypes as C

import numpy as np
import pytest

from oracle import Oracle
from openmmcoul import HipCalcCoulForceKernel, _cabi
from tests import hvp_vjp_reference as hvr
from tests import pbc_hvp_vjp_reference as pvr
from tests.test_gpu_batch_periodic_vjp import _conformations, _counts, _system

REL = ABS = 1e-10


def test_null_handles_are_rejected():
    lib = _cabi.load_library()
    pos, boxes = np.zeros((2, 6, 3)), np.tile(np.eye(3), (2, 1, 1))
    vec, grad = np.ones((2, 2, 6, 3)), np.full((2, 6), 5.0)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    vp = lambda a: C.c_void_p(a.ctypes.data)
    for rc in (lib.cf_compute_batch_periodic_hvp_vjp(None, 2, vp(pos), dp(boxes), 2, vp(vec), vp(vec), vp(grad)),
               lib.cf_compute_batch_periodic_hvp_vjp_host(None, 2, dp(pos), dp(boxes), 2, dp(vec), dp(vec), dp(grad))):
        assert rc == _cabi.CF_ERR_INVALID and b"null" in lib.cf_last_error()
    assert (grad == 5.0).all()


def test_wrapper_argument_checks_need_no_device():
    k = HipCalcCoulForceKernel()   # not initialised: no handle, no device
    k._n = 6
    pos, vec, box = np.zeros((2, 6, 3)), np.ones((2, 2, 6, 3)), np.eye(3)
    for bad in (dict(positions=pos[:, :5], vectors=vec), dict(positions=pos, vectors=vec[:1]),
                dict(positions=pos, vectors=vec[0]), dict(positions=pos, vectors=vec, out_bar=vec[:, :1]),
                dict(positions=pos, vectors=vec.astype(np.float32))):
        with pytest.raises(ValueError):
            k.execute_batch_hvp_vjp_host(**bad, boxes=box)


def test_the_two_steps_agree():
    system, force, pos, box = _system("w22")
    confs, boxes = _conformations("w22", pos, box, 402)
    ref = pvr.Reference(force, *Oracle(force, box).ewald(), boxes[1])   # every fifth atom by a whole box vector
    vecs, ubar = np.random.default_rng(11).normal(size=(2, 1) + pos.shape)
    rows = hvr.grad_rows(ref, confs[1], vecs, ubar)
    hvr.check_groups("w22", rows, hvr.grad_rows(ref, confs[1], vecs, ubar, 2 * hvr.STEP), _counts(force), REL, ABS)
