"""CPU tests of the LJ-gradient boundary (cf_compute_batch_lj_vjp, cf_compute_batch_lj_vjp_host;
include/chargeflux.h): the symbols exist and reject a null handle without touching a device, the API
version is unchanged (the addition is additive), the Python wrappers check shape, dtype and contiguity
before the C call, and BatchedChargeFlux wants sigmas and epsilons together.

They also guard the yardstick of the GPU tests (tests/lj_reference.py): the numpy closed form against
Richardson-extrapolated central differences of the oracle, every LJ parameter of the atoms with
eps > 0, cotangent sets E, F and both.  Bar: the project's VJP bar, max |grad - fd| <= 1e-9 max |grad|
+ 1e-9; measured at <= 7.1e-12 relative (printed)."""
import ctypes as C
import math

import numpy as np
import pytest

from openmmcoul import CoulForce, HipCalcCoulForceKernel, System, _cabi
from openmmcoul import testsystems as ts
from tests import lj_reference as ljr

N = 6
REL, ABS = 1e-9, 1e-9


def test_null_handles_are_rejected():
    lib = _cabi.load_library()
    pos = np.zeros((2, N, 3))
    grad = np.full((2, 2 * N), 5.0)
    p = pos.ctypes.data_as(C.POINTER(C.c_double))
    g = grad.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.cf_compute_batch_lj_vjp(None, 2, C.c_void_p(pos.ctypes.data), None, None, None,
                                       C.c_void_p(grad.ctypes.data)) == _cabi.CF_ERR_INVALID
    assert b"null" in lib.cf_last_error()
    assert lib.cf_compute_batch_lj_vjp_host(None, 2, p, None, None, None, g) == _cabi.CF_ERR_INVALID
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
        k.execute_batch_lj_vjp_host(np.zeros((2, N + 1, 3)))
    with pytest.raises(ValueError):
        k.execute_batch_lj_vjp_host(np.zeros((2, N, 3), dtype=np.float32))
    with pytest.raises(ValueError):
        k.execute_batch_lj_vjp_host(np.zeros((N, 3)))
    with pytest.raises(ValueError):
        k.execute_batch_lj_vjp_host(np.zeros((2, 3, N)).transpose(0, 2, 1))   # right shape, not C-contiguous
    with pytest.raises(ValueError):
        k.execute_batch_lj_vjp_host(pos.tolist())
    # cotangents: another B, wrong trailing shape, dtype, contiguity
    with pytest.raises(ValueError):
        k.execute_batch_lj_vjp_host(pos, energy_bar=np.zeros(3))
    with pytest.raises(ValueError):
        k.execute_batch_lj_vjp_host(pos, forces_bar=np.zeros((3, N, 3)))
    with pytest.raises(ValueError):
        k.execute_batch_lj_vjp_host(pos, forces_bar=np.zeros((2, N + 1, 3)))
    with pytest.raises(ValueError):
        k.execute_batch_lj_vjp_host(pos, energy_bar=np.zeros(2, dtype=np.float32))
    with pytest.raises(ValueError):
        k.execute_batch_lj_vjp_host(pos, forces_bar=np.zeros((2, 3, N)).transpose(0, 2, 1))
    with pytest.raises(ValueError):
        k.execute_batch_lj_vjp_host(pos, energy_bar=np.zeros(4)[::2])
    # boxes: dtype, shape, count
    with pytest.raises(ValueError):
        k.execute_batch_lj_vjp_host(pos, energy_bar=np.zeros(2), boxes=np.eye(3, dtype=np.float32))
    with pytest.raises(ValueError):
        k.execute_batch_lj_vjp_host(pos, energy_bar=np.zeros(2), boxes=np.zeros((3, 3, 3)))
    with pytest.raises(ValueError):
        k.execute_batch_lj_vjp_host(pos, energy_bar=np.zeros(2), boxes=np.zeros((2, 9)))


def test_device_wrapper_rejects_bad_arrays():
    import torch
    k = _uninitialised_kernel()
    f64 = torch.float64
    pos = torch.zeros((2, N, 3), dtype=f64)
    grad = torch.zeros((2, 2 * N), dtype=f64)
    with pytest.raises(ValueError):
        k.execute_batch_lj_vjp_device(torch.zeros((2, N + 1, 3), dtype=f64), grad)
    with pytest.raises(ValueError):
        k.execute_batch_lj_vjp_device(torch.zeros((2, N, 3), dtype=torch.float32), grad)
    with pytest.raises(ValueError):
        k.execute_batch_lj_vjp_device(torch.zeros((2, 3, N), dtype=f64).transpose(1, 2), grad)
    with pytest.raises(ValueError):
        k.execute_batch_lj_vjp_device(np.zeros((2, N, 3)), grad)
    with pytest.raises(ValueError):
        k.execute_batch_lj_vjp_device(pos, grad, energy_bar=torch.zeros(3, dtype=f64))
    with pytest.raises(ValueError):
        k.execute_batch_lj_vjp_device(pos, grad, forces_bar=torch.zeros((3, N, 3), dtype=f64))
    with pytest.raises(ValueError):
        k.execute_batch_lj_vjp_device(pos, grad, forces_bar=torch.zeros((2, N, 3), dtype=torch.float32))
    with pytest.raises(ValueError):
        k.execute_batch_lj_vjp_device(pos, grad, energy_bar=torch.zeros(4, dtype=f64)[::2])
    with pytest.raises(ValueError):
        k.execute_batch_lj_vjp_device(pos, grad, energy_bar=np.zeros(2))
    # grad: (B, 2N) float64 contiguous torch tensor
    with pytest.raises(ValueError):
        k.execute_batch_lj_vjp_device(pos, grad.numpy())
    with pytest.raises(ValueError):
        k.execute_batch_lj_vjp_device(pos, torch.zeros((2, N), dtype=f64))
    with pytest.raises(ValueError):
        k.execute_batch_lj_vjp_device(pos, torch.zeros((3, 2 * N), dtype=f64))
    with pytest.raises(ValueError):
        k.execute_batch_lj_vjp_device(pos, torch.zeros((2, 2 * N), dtype=torch.float32))
    with pytest.raises(ValueError):
        k.execute_batch_lj_vjp_device(pos, torch.zeros((2, 4 * N), dtype=f64)[:, ::2])


def test_fitting_wants_sigmas_and_epsilons_together():
    import torch
    from openmmcoul.fitting import BatchedChargeFlux
    force = CoulForce()
    for _ in range(N):
        force.addParticle(0.0, 0.3, 0.5)
    model = BatchedChargeFlux(_uninitialised_kernel(), force)
    q, pos = torch.zeros(N, dtype=torch.float64), torch.zeros((1, N, 3), dtype=torch.float64)
    none = torch.zeros((0, 2), dtype=torch.float64)
    w = torch.zeros((0, 5), dtype=torch.float64)
    lj = torch.full((N,), 0.3, dtype=torch.float64)
    with pytest.raises(ValueError, match="together"):
        model(q, none, none, w, pos, sigmas=lj)
    with pytest.raises(ValueError, match="together"):
        model(q, none, none, w, pos, epsilons=lj)
    with pytest.raises(ValueError):
        model(q, none, none, w, pos, sigmas=lj, epsilons=lj.to(torch.float32))
    s, e = model.lj_parameters()
    assert s.requires_grad and e.requires_grad and s.dtype == torch.float64
    assert s.tolist() == [0.3] * N and e.tolist() == [0.5] * N


# ---- the reference itself: closed form against the oracle's extrapolated differences ----------------
def _cluster(nw, ni, seed=ts.SEED):
    """The cluster recipe of the batch tests: nw flux waters and ni ions on a jittered lattice."""
    rng = np.random.default_rng(seed + 1000 * nw + ni)
    a = 0.325
    m = max(1, int(math.ceil(max(nw, ni) ** (1.0 / 3.0) - 1e-9)))
    grid = np.array([(i, j, k) for i in range(m) for j in range(m) for k in range(m)], dtype=np.float64)
    wcent = (grid[:nw] + 0.25) * a + rng.uniform(-0.02, 0.02, size=(nw, 3))
    icent = (grid[:ni] + 0.75) * a + rng.uniform(-0.02, 0.02, size=(ni, 3))
    wpos = ts._water_geometry(rng, wcent).reshape(-1, 3)
    force, system = CoulForce(), System()
    for w in range(nw):
        for q, s, e, mass in ((ts.Q_O, ts.SIG_O, ts.EPS_O, 15.999), (ts.Q_H, 0.0, 0.0, 1.008), (ts.Q_H, 0.0, 0.0, 1.008)):
            force.addParticle(q, s, e)
            system.addParticle(mass)
    for w in range(nw):
        ts.add_water(force, 3 * w, w % 2 == 1)
    for i in range(ni):
        force.addParticle(1.0 if i % 2 == 0 else -1.0, 0.3, 0.5)
        system.addParticle(22.99 if i % 2 == 0 else 35.45)
    system.addForce(force)
    return system, force, np.concatenate([wpos, icent])


@pytest.mark.parametrize("name", ["cluster 3+3", "water_box(8, 0.3)"])
def test_closed_form_matches_extrapolated_differences_of_the_oracle(name):
    if name.startswith("cluster"):
        system, force, pos = _cluster(3, 3)
        box = None
    else:
        system, force, pos, box = ts.water_box(8, cutoff=0.3)
        assert ljr.pair_gap_to_cutoff(force, pos, box) > 1e-6   # the moved parameters do not move the pair set
    n = len(pos)
    rng = np.random.default_rng(77)
    eb, fb = rng.normal(size=1), rng.normal(size=(1, n, 3))
    cots = {"E": (eb, None), "F": (None, fb), "EF": (eb, fb)}
    params = ljr.active_parameters(force)
    assert len(params) == 2 * sum(e > 0 for e in force._eps) > 0
    fd = ljr.richardson_fd(force, box, [pos], None if box is None else [box], cots, params)
    for s, (e, f) in cots.items():
        gs, ge = ljr.closed_form(force, pos, box, None if e is None else e[0], None if f is None else f[0])
        g = np.concatenate([gs, ge])
        scale = np.abs(g).max()
        err = np.abs(g[params] - fd[s][0]).max()
        print(f"{name} [{s}]: max|closed - fd| = {err:.3e}, max|grad| = {scale:.3e}, ratio = {err / scale:.3e}")
        assert scale > 1.0
        assert err <= REL * scale + ABS, (name, s, err, scale)
        off = [i for i in range(n) if force._eps[i] == 0.0]
        assert not g[off].any() and not g[[n + i for i in off]].any()
