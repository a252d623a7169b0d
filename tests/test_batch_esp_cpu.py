"""CPU tests of the ESP boundary (cf_compute_batch_esp, cf_compute_batch_esp_vjp, their host forms): a
null handle is rejected without touching a device, and the wrappers check their arrays before the C
call.  They also pin the GPU tests' yardstick (tests/esp_reference.py) on those tests' own inputs: V built
in fp64 from the oracle's charges against the reference V, bar 1e-13 S_p, and the reference gradient
against central differences of its own L (affine in every parameter: h = 1e-2, no truncation error) at
test_batch_dipole_cpu.py's bar, max |grad - fd| <= 1e-9 max |grad| + 1e-9.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import Oracle
from openmmcoul import HipCalcCoulForceKernel, _cabi
from openmmcoul import testsystems as ts
from tests import dipole_reference as dr
from tests import esp_reference as er
from tests.test_gpu_batch_vjp import _cluster, _conformations

N, M = 6, 5


def test_null_handles_are_rejected():
    lib = _cabi.load_library()
    pos, pts = np.zeros((2, N, 3)), np.ones((2, M, 3))
    out = np.full((2, N + M), 5.0)
    p, r, o = (a.ctypes.data_as(C.POINTER(C.c_double)) for a in (pos, pts, out))
    vp, vr, vo = (C.c_void_p(a.ctypes.data) for a in (pos, pts, out))
    for rc in (lib.cf_compute_batch_esp(None, 2, vp, M, vr, vo, None),
               lib.cf_compute_batch_esp_host(None, 2, p, M, r, o, None),
               lib.cf_compute_batch_esp_vjp(None, 2, vp, M, vr, None, vo),
               lib.cf_compute_batch_esp_vjp_host(None, 2, p, M, r, None, o)):
        assert rc == _cabi.CF_ERR_INVALID
        assert b"null" in lib.cf_last_error()
    assert (out == 5.0).all()
    assert lib.cf_api_version() == 4


def test_wrappers_reject_bad_arrays():
    k = HipCalcCoulForceKernel()   # no device here: the wrappers must raise before they reach the (null) handle
    k._n = N
    pos, pts = np.zeros((2, N, 3)), np.ones((2, M, 3))
    bad_points = (np.ones((2, M)), np.ones((3, M, 3)), np.ones((2, M, 4)), np.ones((2, M, 3), dtype=np.float32),
                  np.ones((2, 3, M)).transpose(0, 2, 1), pts.tolist())
    for call in (k.execute_batch_esp_host, k.execute_batch_esp_vjp_host):
        for bad in bad_points:
            with pytest.raises(ValueError):
                call(pos, bad)
        for bad in (np.zeros((N, 3)), np.zeros((2, N, 3), dtype=np.float32), np.zeros((2, 3, N)).transpose(0, 2, 1)):
            with pytest.raises(ValueError):
                call(bad, pts)
    for bad in (np.zeros((2, M + 1)), np.zeros((3, M)), np.zeros((2, M), dtype=np.float32), np.zeros((2, 2 * M))[:, ::2]):
        with pytest.raises(ValueError):   # a cotangent for another npts or B, float32, not contiguous
            k.execute_batch_esp_vjp_host(pos, pts, esp_bar=bad)


@pytest.mark.parametrize("nw,ni,npts", [(1, 0, 77), (0, 5, 300), (2, 1, 77), (21, 7, 300)])
def test_reference_is_pinned(nw, ni, npts):
    system, force, pos = _cluster(nw, ni)
    seed = 177 + nw + ni                                     # the inputs of test_gpu_batch_esp.py's _case
    confs = _conformations(pos, seed)
    points = ts.probe_points(confs, npts, seed + 500 + npts)[0]
    vbar = np.random.default_rng(seed + 31).normal(size=(len(confs), npts))
    o = Oracle(force)
    theta = dr.flat_parameters(force)
    for conf, pts, vb in zip(confs, points, vbar):
        r = er.evaluate(force, conf, pts, vb)
        q = o.execute(conf, None, False, False)["charges"]
        dist = np.sqrt(((pts[:, None] - conf[None]) ** 2).sum(axis=2))
        err = (np.abs(er.KE * ((1 / dist) @ q) - r["V"]) / r["S_V"]).max()
        fd = np.zeros_like(theta)
        for p in range(len(theta)):
            tp, tm = theta.copy(), theta.copy()
            tp[p] += 1e-2
            tm[p] -= 1e-2
            fd[p] = (er.evaluate(force, conf, pts, vb, theta=tp)["L"] - er.evaluate(force, conf, pts, vb, theta=tm)["L"]) / 2e-2
        worst, scale = np.abs(r["grad"] - fd).max(), np.abs(r["grad"]).max()
        print(f"{nw}+{ni}, M = {npts}: max|V - V(oracle q)|/S = {err:.3e}, max|grad - fd| = {worst:.3e}, max|grad| = {scale:.3e}")
        assert err <= 1e-13
        assert worst <= 1e-9 * scale + 1e-9
