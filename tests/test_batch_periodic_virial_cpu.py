"""CPU tests of the periodic virial boundary (cf_compute_batch_periodic_virial and its host form;
include/chargeflux.h): the symbols exist and reject a null handle without touching a device.

They also guard the yardstick of the GPU tests (tests/pbc_virial_reference.py) on `ions`, `w22` and
`aniso` of tests/test_gpu_batch_periodic_vjp.py:
  - its real energy at zero strain against the oracle's, the project's fp64 energy bar
    |dE| <= 1e-9 |E| + 1e-8;
  - its virial is symmetric.  The nine components are nine separate complex steps through sums of
    N^2 pair and N khalf reciprocal terms, each rounded to eps relative to at most S (the sum over the
    parts of the part's largest entry): bar 10 eps (N + khalf) S;
  - its trace against a central difference of its own energy under the isotropic scaling
    x -> (1 + l) x, box -> (1 + l) box at the images and pair set of l = 0, h = 1e-4: dE/dl = -tr.
    Two error terms, both computed here: round-off eps sum|E_part| / h and the h^2 truncation, taken
    from a second step as |fd(2h) - fd(h)| / 3; the bar is 10 times the larger.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import Oracle
from openmmcoul import _cabi
from tests import pbc_virial_reference as vr
from tests.test_gpu_batch_periodic_vjp import _system

H_FD = 1e-4
EPS = np.finfo(np.float64).eps / 2


def test_symbols_and_null_handles():
    lib = _cabi.load_library()
    assert hasattr(lib, "cf_compute_batch_periodic_virial") and hasattr(lib, "cf_compute_batch_periodic_virial_host")
    pos, boxes = np.zeros((2, 6, 3)), np.tile(np.eye(3), (2, 1, 1))
    vir = np.full((2, 3, 3), 5.0)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    vp = lambda a: C.c_void_p(a.ctypes.data)
    for rc in (lib.cf_compute_batch_periodic_virial(None, 2, vp(pos), dp(boxes), 3, None, None, None, vp(vir)),
               lib.cf_compute_batch_periodic_virial_host(None, 2, dp(pos), dp(boxes), 3, None, None, None, dp(vir)),
               lib.cf_compute_batch_periodic_virial(None, 2, vp(pos), dp(boxes), 3, None, None, None, None)):
        assert rc == _cabi.CF_ERR_INVALID and b"null" in lib.cf_last_error()
    assert (vir == 5.0).all()


@functools.lru_cache(maxsize=None)
def _case(name):
    system, force, pos, box = _system(name)
    o = Oracle(force, box)
    ref = vr.Reference(force, *o.ewald())
    return o, ref, pos, box, ref.virial_parts(pos, box)


@pytest.mark.parametrize("name", ["ions", "w22", "aniso"])
def test_reference_energy_matches_the_oracle(name):
    o, ref, pos, box, _ = _case(name)
    e, e_ref = sum(ref.energy_parts(pos, box).values()), o.execute(pos, box)["energy"]
    print(f"{name}: E = {e:.12f}, oracle {e_ref:.12f}, |dE| = {abs(e - e_ref):.3e}")
    assert abs(e - e_ref) <= 1e-9 * abs(e_ref) + 1e-8


@pytest.mark.parametrize("name", ["ions", "w22", "aniso"])
def test_reference_virial_is_symmetric_and_its_trace_is_the_volume_derivative(name):
    o, ref, pos, box, v = _case(name)
    scale = sum(np.abs(v[p]).max() for p in vr.PARTS)
    asym = np.abs(v["total"] - v["total"].T).max()
    bar = 10 * EPS * (len(pos) + len(ref.kint)) * scale
    print(f"{name}: max|V - V^T| = {asym:.3e}, S = {scale:.3e}, bar = {bar:.3e}")
    assert asym <= bar
    energy = lambda l: ref.energy_parts((1 + l) * pos, (1 + l) * box, at=(pos, box))
    fd = lambda h: (sum(energy(h).values()) - sum(energy(-h).values())) / (2 * h)
    fd1, fd2 = fd(H_FD), fd(2 * H_FD)
    roundoff = EPS * sum(abs(e) for e in energy(0.0).values()) / H_FD
    trunc = abs(fd2 - fd1) / 3
    err = abs(-np.trace(v["total"]) - fd1)
    print(f"{name}: tr = {np.trace(v['total']):.9e}, round-off = {roundoff:.3e}, truncation = {trunc:.3e}, "
          f"|tr + dE/dl| = {err:.3e}")
    assert err <= 10 * max(roundoff, trunc)
