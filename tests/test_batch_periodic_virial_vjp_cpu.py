"""CPU tests of cf_compute_batch_periodic_virial_vjp and its host form (include/chargeflux.h): the symbols
exist and reject a null handle without touching a device or an output; the Python wrappers check their
arrays before the C call.  They also guard the GPU tests' yardstick (tests/pbc_virial_grad_reference.py)
on frame 1 (molecules split across images) of `ions` and `w22` of test_gpu_batch_periodic_vjp.py:
  - L by one complex step along the strain equals W_bar : virial of the nine-step reference, to
    10 eps (N + khalf) |W_bar| S (test_batch_periodic_virial_cpu.py's bar for that reference's rounding);
  - central differences with steps h_p and 2 h_p agree (L is exactly quadratic in a parameter): their
    worst disagreement relative to G, printed, is the reference's own noise and must be at least ten
    times below the GPU bar 1e-9 G + 1e-9.  Observed: 3.2e-14 G (ions), 1.7e-14 G (w22, one parameter
    in three and the ends of every group).
"""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import Oracle
from openmmcoul import HipCalcCoulForceKernel, _cabi
from tests import pbc_virial_grad_reference as gr
from tests import pbc_virial_reference as vr
from tests.test_gpu_batch_periodic_vjp import SYSTEMS, _conformations, _counts, _system

N = 6
EPS = np.finfo(np.float64).eps / 2
W_BAR = np.array([[0.7, -1.1, 0.4], [0.3, -0.5, 0.9], [-0.6, 0.2, 1.3]])


def test_symbols_and_null_handles():
    lib = _cabi.load_library()
    for name in ("cf_compute_batch_periodic_virial", "cf_compute_batch_periodic_virial_host",
                 "cf_compute_batch_periodic_virial_vjp", "cf_compute_batch_periodic_virial_vjp_host"):
        assert hasattr(lib, name)
    assert lib.cf_api_version() == 4
    pos, boxes, wb = np.zeros((2, N, 3)), np.tile(np.eye(3), (2, 1, 1)), np.ones((2, 3, 3))
    grad, ljg = np.full((2, N), 5.0), np.full((2, 2 * N), 5.0)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    vp = lambda a: C.c_void_p(a.ctypes.data)
    for rc in (lib.cf_compute_batch_periodic_virial_vjp(None, 2, vp(pos), dp(boxes), vp(wb), vp(grad), vp(ljg)),
               lib.cf_compute_batch_periodic_virial_vjp_host(None, 2, dp(pos), dp(boxes), dp(wb), dp(grad), dp(ljg)),
               lib.cf_compute_batch_periodic_virial_vjp(None, 2, vp(pos), dp(boxes), None, None, None)):
        assert rc == _cabi.CF_ERR_INVALID and b"null" in lib.cf_last_error()
    assert (grad == 5.0).all() and (ljg == 5.0).all()


BAD = [  # (positions, boxes, virial_bar) as numpy arrays for 2 conformations of N atoms
    (np.zeros((2, N + 1, 3)), np.eye(3), None),
    (np.zeros((2, N, 3), dtype=np.float32), np.eye(3), None),
    (np.zeros((2, N, 3)), np.zeros((3, 3, 3)), None),
    (np.zeros((2, N, 3)), np.zeros((2, 3, 3), dtype=np.float32), None),
    (np.zeros((2, N, 3)), np.eye(3), np.zeros((2, 9))),
    (np.zeros((2, N, 3)), np.eye(3), np.zeros((3, 3, 3))),
    (np.zeros((2, N, 3)), np.eye(3), np.zeros((2, 3, 3)).transpose(0, 2, 1)),
    (np.zeros((2, N, 3)), np.eye(3), np.zeros((2, 3, 3), dtype=np.float32)),
]


@pytest.mark.parametrize("pos, boxes, wb", BAD, ids=range(len(BAD)))
def test_wrappers_reject_bad_arrays(pos, boxes, wb):
    import torch
    k = HipCalcCoulForceKernel()   # no device here: the wrappers must raise before they reach the (null) handle
    k._n = N
    with pytest.raises(ValueError):
        k.execute_batch_virial_vjp_host(pos, boxes, wb)
    as_t = lambda a: None if a is None else (torch.from_numpy(a) if a.flags.c_contiguous else torch.from_numpy(a.copy()).mT)
    with pytest.raises(ValueError):
        k.execute_batch_virial_vjp_device(as_t(pos), boxes, None, as_t(wb), None)


@pytest.mark.parametrize("name, shape, dtype", [("grad", (2, N), "float32"), ("grad", (3, N), "float64"),
                                               ("grad", (2 * N,), "float64"), ("grad", (N, 2), "mT"),
                                               ("lj_grad", (2, N), "float64"), ("lj_grad", (2, 2 * N), "float32"),
                                               ("lj_grad", (3, 2 * N), "float64"), ("lj_grad", (2 * N, 2), "mT")])
def test_device_wrapper_rejects_bad_outputs(name, shape, dtype):
    import torch
    k = HipCalcCoulForceKernel()   # grad's dtype, layout and rows are checked before the handle is asked for P
    k._n = N
    out = torch.zeros(shape, dtype=torch.float64).mT if dtype == "mT" else torch.zeros(shape, dtype=getattr(torch, dtype))
    with pytest.raises(ValueError):
        k.execute_batch_virial_vjp_device(torch.zeros((2, N, 3), dtype=torch.float64), np.eye(3), **{name: out})


@functools.lru_cache(maxsize=None)
def _case(name):
    system, force, pos, box = _system(name)
    confs, boxes = _conformations(name, pos, box, 400 + SYSTEMS.index(name))
    return force, vr.Reference(force, *Oracle(force, box).ewald()), confs[1], boxes[1]


@pytest.mark.parametrize("name", ["ions", "w22"])
def test_reference_loss_is_the_contraction_of_the_reference_virial(name):
    force, ref, x, box = _case(name)
    v = ref.virial_parts(x, box)
    loss = gr.total(gr.loss_parts(ref, x, box, W_BAR))
    bar = 10 * EPS * (len(x) + len(ref.kint)) * np.abs(W_BAR).sum() * sum(np.abs(v[p]).max() for p in vr.PARTS)
    print(f"{name}: L = {loss:.12e}, W_bar : virial = {np.sum(W_BAR * v['total']):.12e}, bar = {bar:.3e}")
    assert abs(loss - np.sum(W_BAR * v["total"])) <= bar


@pytest.mark.parametrize("name", ["ions", "w22"])
def test_reference_gradient_does_not_depend_on_the_step(name):
    force, ref, x, box = _case(name)
    params = gr.strided(_counts(force), 1 if name == "ions" else 3)
    g1, g2 = (gr.theta_gradient(ref, x, box, W_BAR, params, s) for s in (gr.H_FD, 2 * gr.H_FD))
    noise, G = np.abs(gr.total(g1) - gr.total(g2)).max(), gr.scale(g1)
    print(f"{name}: {len(params)} parameters, max|grad(h) - grad(2h)| = {noise:.3e}, G = {G:.3e}, ratio = {noise / G:.3e}")
    assert np.abs(gr.total(g1)).max() > 0 and 10 * noise <= 1e-9 * G + 1e-9
