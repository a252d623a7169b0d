"""CPU tests of the dipole / polar-tensor boundary (cf_compute_batch_dipole, cf_compute_batch_dipole_vjp
and their host forms; include/chargeflux.h): the symbols exist and reject a null handle without
touching a device, and the Python wrappers check shape, dtype and contiguity before the C call.

They also guard the yardstick of the GPU tests (tests/dipole_reference.py), on the clusters (1 water,
0 ions), (0, 5), (2, 1) and (21, 7) of the batch tests, B = 3 conformations each:
  - charges and dipole against the oracle's charges, bar 1e-13 (observed <= 5.6e-16);
  - P against central differences over the positions of sum_a q_a(x) x_a built from the oracle's
    charges, h = 1e-6 nm, bar 2e-9: the error is finite-difference round-off, eps |mu| / h, observed
    5.8e-11, 8.2e-11, 6.9e-11 and 2.1e-10 at max |P| = 1, and the bar is 10 times the worst
    (h = 1e-5 would add 2e-9 of truncation);
  - sum_b P_b = (sum q) I to 1e-13, and a translation d moves mu by (sum q) d and leaves P unchanged;
  - the reference gradient against central differences over each parameter of the reference's own
    L, h = 1e-2 (L is affine in every parameter: no truncation error), at the project's bar
    max |grad - fd| <= 1e-9 max |grad| + 1e-9.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import Oracle
from openmmcoul import HipCalcCoulForceKernel, _cabi
from tests import dipole_reference as dr
from tests.test_gpu_batch_vjp import _cluster, _conformations

N = 6
SIZES = [(1, 0), (0, 5), (2, 1), (21, 7)]
H_POS = 1e-6
H_PAR = 1e-2
REL, ABS = 1e-9, 1e-9


def test_null_handles_are_rejected():
    lib = _cabi.load_library()
    pos = np.zeros((2, N, 3))
    out = np.full((2, N, 3, 3), 5.0)
    p = pos.ctypes.data_as(C.POINTER(C.c_double))
    o = out.ctypes.data_as(C.POINTER(C.c_double))
    vp, vo = C.c_void_p(pos.ctypes.data), C.c_void_p(out.ctypes.data)
    for rc in (lib.cf_compute_batch_dipole(None, 2, vp, None, vo, None),
               lib.cf_compute_batch_dipole_host(None, 2, p, None, o, None),
               lib.cf_compute_batch_dipole_vjp(None, 2, vp, None, None, vo),
               lib.cf_compute_batch_dipole_vjp_host(None, 2, p, None, None, o)):
        assert rc == _cabi.CF_ERR_INVALID
        assert b"null" in lib.cf_last_error()
    assert (out == 5.0).all()
    assert lib.cf_api_version() == 4


def _uninitialised_kernel():
    # no device here: the wrappers must raise before they reach the (null) handle
    k = HipCalcCoulForceKernel()
    k._n = N
    return k


def test_host_wrappers_reject_bad_arrays():
    k = _uninitialised_kernel()
    pos = np.zeros((2, N, 3))
    for call in (k.execute_batch_dipole_host, k.execute_batch_dipole_vjp_host):
        with pytest.raises(ValueError):
            call(np.zeros((2, N + 1, 3)))
        with pytest.raises(ValueError):
            call(np.zeros((2, N, 3), dtype=np.float32))
        with pytest.raises(ValueError):
            call(np.zeros((N, 3)))
        with pytest.raises(ValueError):
            call(np.zeros((2, 3, N)).transpose(0, 2, 1))   # right shape, not C-contiguous
        with pytest.raises(ValueError):
            call(pos.tolist())
    # cotangents: another B, wrong trailing shape, dtype, contiguity
    with pytest.raises(ValueError):
        k.execute_batch_dipole_vjp_host(pos, dipole_bar=np.zeros((3, 3)))
    with pytest.raises(ValueError):
        k.execute_batch_dipole_vjp_host(pos, dipole_bar=np.zeros((2, 4)))
    with pytest.raises(ValueError):
        k.execute_batch_dipole_vjp_host(pos, dipole_bar=np.zeros((2, 3), dtype=np.float32))
    with pytest.raises(ValueError):
        k.execute_batch_dipole_vjp_host(pos, apt_bar=np.zeros((2, N, 9)))
    with pytest.raises(ValueError):
        k.execute_batch_dipole_vjp_host(pos, apt_bar=np.zeros((3, N, 3, 3)))
    with pytest.raises(ValueError):
        k.execute_batch_dipole_vjp_host(pos, apt_bar=np.zeros((2, N, 3, 6))[..., ::2])
    with pytest.raises(ValueError):
        k.execute_batch_dipole_vjp_host(pos, apt_bar=np.zeros((2, N, 3, 3)).tolist())


def test_device_wrappers_reject_bad_arrays():
    import torch
    k = _uninitialised_kernel()
    f64 = torch.float64
    pos = torch.zeros((2, N, 3), dtype=f64)
    grad = torch.zeros((2, N), dtype=f64)
    for call in (k.execute_batch_dipole_device, lambda p: k.execute_batch_dipole_vjp_device(p, grad)):
        with pytest.raises(ValueError):
            call(torch.zeros((2, N + 1, 3), dtype=f64))
        with pytest.raises(ValueError):
            call(torch.zeros((2, N, 3), dtype=torch.float32))
        with pytest.raises(ValueError):
            call(torch.zeros((2, 3, N), dtype=f64).transpose(1, 2))
        with pytest.raises(ValueError):
            call(np.zeros((2, N, 3)))
    # outputs of the forward call
    with pytest.raises(ValueError):
        k.execute_batch_dipole_device(pos, dipoles=torch.zeros((3, 3), dtype=f64))
    with pytest.raises(ValueError):
        k.execute_batch_dipole_device(pos, dipoles=torch.zeros((2, 3), dtype=torch.float32))
    with pytest.raises(ValueError):
        k.execute_batch_dipole_device(pos, apts=torch.zeros((2, N, 9), dtype=f64))
    with pytest.raises(ValueError):
        k.execute_batch_dipole_device(pos, apts=np.zeros((2, N, 3, 3)))
    with pytest.raises(ValueError):
        k.execute_batch_dipole_device(pos, charges=torch.zeros((2, N + 1), dtype=f64))
    with pytest.raises(ValueError):
        k.execute_batch_dipole_device(pos, charges=torch.zeros((2, 2 * N), dtype=f64)[:, ::2])
    # cotangents and grad of the VJP call
    with pytest.raises(ValueError):
        k.execute_batch_dipole_vjp_device(pos, grad, dipole_bar=torch.zeros((3, 3), dtype=f64))
    with pytest.raises(ValueError):
        k.execute_batch_dipole_vjp_device(pos, grad, dipole_bar=np.zeros((2, 3)))
    with pytest.raises(ValueError):
        k.execute_batch_dipole_vjp_device(pos, grad, apt_bar=torch.zeros((2, N, 3, 3), dtype=torch.float32))
    with pytest.raises(ValueError):
        k.execute_batch_dipole_vjp_device(pos, grad, apt_bar=torch.zeros((2, N, 3), dtype=f64))
    with pytest.raises(ValueError):
        k.execute_batch_dipole_vjp_device(pos, grad.numpy())


# ---- the reference itself ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(nw, ni):
    system, force, pos = _cluster(nw, ni)
    confs = _conformations(pos, 177 + nw + ni)
    return force, confs, [dr.evaluate(force, c) for c in confs]


@pytest.mark.parametrize("nw,ni", SIZES)
def test_reference_charges_and_dipole_match_the_oracle(nw, ni):
    force, confs, ref = _case(nw, ni)
    o = Oracle(force)
    worst = 0.0
    for conf, r in zip(confs, ref):
        q = o.execute(conf, None)["charges"]
        worst = max(worst, np.abs(r["q"] - q).max(), np.abs(r["mu"] - q @ conf).max())
    print(f"{nw}+{ni}: max|q - oracle|, max|mu - oracle| <= {worst:.3e}")
    assert worst <= 1e-13


@pytest.mark.parametrize("nw,ni", SIZES)
def test_reference_polar_tensor_matches_position_differences_of_the_oracle(nw, ni):
    force, confs, ref = _case(nw, ni)
    o = Oracle(force)
    n = confs.shape[1]
    dipole = lambda x: o.execute(x, None, False, False)["charges"] @ x
    worst = scale = 0.0
    for conf, r in zip(confs, ref):
        fd = np.zeros((n, 3, 3))
        for b in range(n):
            for be in range(3):
                xp, xm = conf.copy(), conf.copy()
                xp[b, be] += H_POS
                xm[b, be] -= H_POS
                fd[b, :, be] = (dipole(xp) - dipole(xm)) / (2 * H_POS)
        worst = max(worst, np.abs(r["P"] - fd).max())
        scale = max(scale, np.abs(r["P"]).max())
    print(f"{nw}+{ni}: max|P - fd| = {worst:.3e}, max|P| = {scale:.3e}")
    assert worst <= 2e-9


@pytest.mark.parametrize("nw,ni", SIZES)
def test_reference_sum_rule_and_translation(nw, ni):
    force, confs, ref = _case(nw, ni)
    d = np.array([0.3, -0.7, 0.2])
    for conf, r in zip(confs, ref):
        total = r["q"].sum()
        assert np.abs(r["P"].sum(axis=0) - total * np.eye(3)).max() <= 1e-13
        moved = dr.evaluate(force, conf + d)
        # at most 70 terms of size <= ~2 nm e per sum: round-off below 70 * 2 * 1.1e-16 = 1.6e-14
        assert np.abs(moved["mu"] - (r["mu"] + total * d)).max() <= 1e-13
        assert np.abs(moved["P"] - r["P"]).max() <= 1e-13
        assert np.abs(moved["q"] - r["q"]).max() <= 1e-13


@pytest.mark.parametrize("nw,ni", SIZES)
def test_reference_gradient_matches_parameter_differences_of_its_own_scalar(nw, ni):
    force, confs, _ = _case(nw, ni)
    n = confs.shape[1]
    rng = np.random.default_rng(31 + nw + ni)
    mb, pb = rng.normal(size=(len(confs), 3)), rng.normal(size=(len(confs), n, 3, 3))
    theta = dr.flat_parameters(force)
    for s, (use_m, use_p) in {"mu": (True, False), "P": (False, True), "both": (True, True)}.items():
        worst = scale = 0.0
        for b, conf in enumerate(confs):
            cot = (mb[b] if use_m else None, pb[b] if use_p else None)
            g = dr.evaluate(force, conf, *cot)["grad"]
            fd = np.zeros_like(g)
            for p in range(len(theta)):
                tp, tm = theta.copy(), theta.copy()
                tp[p] += H_PAR
                tm[p] -= H_PAR
                fd[p] = (dr.evaluate(force, conf, *cot, theta=tp)["L"]
                         - dr.evaluate(force, conf, *cot, theta=tm)["L"]) / (2 * H_PAR)
            worst, scale = max(worst, np.abs(g - fd).max()), max(scale, np.abs(g).max())
        print(f"{nw}+{ni} [{s}]: max|grad - fd| = {worst:.3e}, max|grad| = {scale:.3e}")
        assert worst <= REL * scale + ABS, (nw, ni, s, worst, scale)
