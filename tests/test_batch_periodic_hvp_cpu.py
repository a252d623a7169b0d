"""CPU tests of the periodic Hessian-vector boundary (cf_compute_batch_periodic_hvp and its host
form; include/chargeflux.h): the symbols exist and reject a null handle without touching a device.

They also guard the yardstick of the GPU tests (tests/pbc_hvp_reference.py) on 8 waters (every second
one bond + angle) in a cubic box (`ortho`) and in a sheared box with atoms of two molecules moved by
whole box vectors, so that molecules are split across images (`tric`).
  - The reference's forces at real positions against the oracle's.  Both add N pair terms and khalf
    k-space terms per atom in fp64, each rounded to eps = 1.1e-16 relative to at most max|F|: the bar is
    10 eps (N + khalf) max|F| (khalf = 1098: ortho 1.7e-9, tric 5.2e-9 kJ/mol/nm); observed 6.7e-12 and 9.9e-12.
  - The reference's H v against central differences of the ORACLE's forces along a seeded N(0, 1)
    direction, h = 1e-5 nm.  Two error terms, both computed in the test: the oracle's round-off
    eps max|F| / h, and the h^2 truncation, taken from a second step as max|fd(2h) - fd(h)| / 3.  The bar
    is 10 times the larger.  Observed (kJ/mol/nm^2): ortho round-off 1.5e-8, truncation 3.16e-2,
    max|Hv - fd| 3.16e-2; tric 4.6e-8, 3.39e-2, 3.39e-2 (max|Hv| 1.1e5 and 1.3e5: 2.8e-7 relative).
"""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import Oracle
from openmmcoul import _cabi
from openmmcoul import testsystems as ts
from tests import pbc_hvp_reference as pr

H_FD = 1e-5
EPS = np.finfo(np.float64).eps / 2


def test_null_handles_are_rejected():
    lib = _cabi.load_library()
    assert hasattr(lib, "cf_compute_batch_periodic_hvp") and hasattr(lib, "cf_compute_batch_periodic_hvp_host")
    pos, boxes = np.zeros((2, 6, 3)), np.tile(np.eye(3), (2, 1, 1))
    vec, out = np.ones((2, 2, 6, 3)), np.full((2, 2, 6, 3), 5.0)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    vp = lambda a: C.c_void_p(a.ctypes.data)
    for rc in (lib.cf_compute_batch_periodic_hvp(None, 2, vp(pos), dp(boxes), 2, vp(vec), vp(out)),
               lib.cf_compute_batch_periodic_hvp_host(None, 2, dp(pos), dp(boxes), 2, dp(vec), dp(out))):
        assert rc == _cabi.CF_ERR_INVALID
        assert b"null" in lib.cf_last_error()
    assert (out == 5.0).all()
    assert lib.cf_api_version() == 4


@functools.lru_cache(maxsize=None)
def _case(name):
    if name == "ortho":
        system, force, pos, box = ts.water_box(8, cutoff=0.3, every_bond_angle=2)
    else:
        system, force, pos, box = ts.triclinic_water_box(8, cutoff=0.29, every_bond_angle=2)
        pos = pos.copy()
        pos[1] += box[2]           # a hydrogen of molecule 0 one c vector up
        pos[9] -= box[1]           # the oxygen of molecule 3 one b vector down
        assert box[1, 0] != 0 and box[2, 0] != 0 and box[2, 1] != 0
    o = Oracle(force, box)
    ref = pr.Reference(force, *o.ewald())
    return o, ref, pos, box


@pytest.mark.parametrize("name", ["ortho", "tric"])
def test_reference_forces_match_the_oracle(name):
    o, ref, pos, box = _case(name)
    f = o.execute(pos, box)["forces"]
    err, scale = np.abs(ref.forces(pos, box) - f).max(), np.abs(f).max()
    bar = 10 * EPS * (len(pos) + len(ref.kint)) * scale
    print(f"{name}: max|F - oracle| = {err:.3e}, max|F| = {scale:.3e}, khalf = {len(ref.kint)}, bar = {bar:.3e}")
    assert err <= bar


@pytest.mark.parametrize("name", ["ortho", "tric"])
def test_reference_hv_matches_central_differences_of_the_oracle(name):
    o, ref, pos, box = _case(name)
    v = np.random.default_rng(61 + len(name)).normal(size=pos.shape)
    forces = lambda x: o.execute(x, box)["forces"]
    fd = lambda h: -(forces(pos + h * v) - forces(pos - h * v)) / (2 * h)
    hv, fd1, fd2 = ref.hv(pos, box, v), fd(H_FD), fd(2 * H_FD)
    roundoff = EPS * np.abs(forces(pos)).max() / H_FD
    trunc = np.abs(fd2 - fd1).max() / 3
    err = np.abs(hv - fd1).max()
    print(f"{name}: round-off = {roundoff:.3e}, truncation = {trunc:.3e}, max|Hv - fd| = {err:.3e}, "
          f"max|Hv| = {np.abs(hv).max():.3e}")
    assert err <= 10 * max(roundoff, trunc)
