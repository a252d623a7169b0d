"""CPU tests of the Hessian-vector boundary (cf_compute_batch_hvp and its host form;
include/chargeflux.h): the symbols exist and reject a null handle without touching a device, and the
Python wrappers check shape, dtype and contiguity before the C call.

They also guard the yardstick of the GPU tests (tests/hvp_reference.py: the complex step through a
numpy restatement of the forces), on the clusters (2 waters, 1 ion) and (21, 7) of the batch tests,
B = 3 conformations each:
  - the reference's forces at real positions against the oracle's, bar 1e-9 max|F| + 1e-9 (observed
    <= 3.9e-12 at max|F| = 2.4e3);
  - the reference's H v against central differences of the ORACLE's forces along v, h = 1e-5 nm, two
    seeded N(0, 1) directions per conformation.  The expected error is round-off eps max|F| / h
    (1.1e-16 * 2e3 / 1e-5 = 2e-8) plus the h^2 truncation of the difference, which dominates:
    observed max|Hv - fd| / max|Hv| = 2.1e-7 on (2, 1) and 3.3e-7 on (21, 7).  The bar is 10 times
    the worst, 3.3e-6 max|Hv| (the margin covers libm differences between hosts);
  - symmetry, |u.(Hv) - v.(Hu)| <= 1e-12 |u| |Hv|, and the three rigid translations as null vectors
    of H to 1e-9 max|H|, max|H| from the reference's full Hessian of (2, 1).
"""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import Oracle
from openmmcoul import HipCalcCoulForceKernel, _cabi
from tests import hvp_reference as hr
from tests.test_gpu_batch_vjp import _cluster, _conformations

N = 6
SIZES = [(2, 1), (21, 7)]
H_FD = 1e-5
FD_BAR = 3.3e-6   # relative to max|Hv|: 10 x the observed 3.3e-7 (see above)


def test_null_handles_are_rejected():
    lib = _cabi.load_library()
    assert hasattr(lib, "cf_compute_batch_hvp") and hasattr(lib, "cf_compute_batch_hvp_host")
    pos = np.zeros((2, N, 3))
    vec = np.ones((2, 2, N, 3))
    out = np.full((2, 2, N, 3), 5.0)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    vp = lambda a: C.c_void_p(a.ctypes.data)
    for rc in (lib.cf_compute_batch_hvp(None, 2, vp(pos), 2, vp(vec), vp(out)),
               lib.cf_compute_batch_hvp_host(None, 2, dp(pos), 2, dp(vec), dp(out))):
        assert rc == _cabi.CF_ERR_INVALID
        assert b"null" in lib.cf_last_error()
    assert (out == 5.0).all()
    assert lib.cf_api_version() == 4


def _uninitialised_kernel():
    # no device here: the wrappers must raise before they reach the (null) handle
    k = HipCalcCoulForceKernel()
    k._n = N
    return k


def test_host_wrapper_rejects_bad_arrays():
    k = _uninitialised_kernel()
    pos, vec = np.zeros((2, N, 3)), np.zeros((2, 3, N, 3))
    bad_vectors = [np.zeros((2, N, 3)),                                  # no K axis
                   np.zeros((2, 3, N + 1, 3)), np.zeros((2, 3, N, 2)),   # not (B,K,N,3)
                   np.zeros((3, 3, N, 3)),                               # another B
                   np.zeros((2, 3, N, 3), dtype=np.float32),
                   np.zeros((2, 3, 3, N)).transpose(0, 1, 3, 2),         # right shape, not C-contiguous
                   vec.tolist()]
    for v in bad_vectors:
        with pytest.raises(ValueError):
            k.execute_batch_hvp_host(pos, v)
    for p in (np.zeros((2, N + 1, 3)), np.zeros((N, 3)), np.zeros((2, N, 3), dtype=np.float32),
              np.zeros((2, 3, N)).transpose(0, 2, 1), pos.tolist()):
        with pytest.raises(ValueError):
            k.execute_batch_hvp_host(p, vec)
        with pytest.raises(ValueError):
            k.hessians_host(p)


def test_device_wrapper_rejects_bad_arrays():
    import torch
    k = _uninitialised_kernel()
    f64 = torch.float64
    pos, vec = torch.zeros((2, N, 3), dtype=f64), torch.zeros((2, 3, N, 3), dtype=f64)
    bad_vectors = [torch.zeros((2, N, 3), dtype=f64), torch.zeros((2, 3, N + 1, 3), dtype=f64),
                   torch.zeros((3, 3, N, 3), dtype=f64), torch.zeros((2, 3, N, 3), dtype=torch.float32),
                   torch.zeros((2, 3, 3, N), dtype=f64).transpose(2, 3), np.zeros((2, 3, N, 3))]
    for v in bad_vectors:
        with pytest.raises(ValueError):
            k.execute_batch_hvp_device(pos, v)
    for p in (torch.zeros((2, N + 1, 3), dtype=f64), torch.zeros((2, N, 3), dtype=torch.float32),
              torch.zeros((2, 3, N), dtype=f64).transpose(1, 2), np.zeros((2, N, 3))):
        with pytest.raises(ValueError):
            k.execute_batch_hvp_device(p, vec)
    for o in (torch.zeros((2, 2, N, 3), dtype=f64), torch.zeros((3, 3, N, 3), dtype=f64),
              torch.zeros((2, 3, N, 3), dtype=torch.float32), torch.zeros((2, 3, N, 6), dtype=f64)[..., ::2],
              np.zeros((2, 3, N, 3))):
        with pytest.raises(ValueError):
            k.execute_batch_hvp_device(pos, vec, out=o)


# ---- the reference itself ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(nw, ni):
    system, force, pos = _cluster(nw, ni)
    return force, _conformations(pos, 177 + nw + ni), hr.Reference(force)


@pytest.mark.parametrize("nw,ni", SIZES)
def test_reference_forces_match_the_oracle(nw, ni):
    force, confs, ref = _case(nw, ni)
    o = Oracle(force)
    worst = scale = 0.0
    for conf in confs:
        f = o.execute(conf, None)["forces"]
        worst, scale = max(worst, np.abs(ref.forces(conf) - f).max()), max(scale, np.abs(f).max())
    print(f"{nw}+{ni}: max|F - oracle| = {worst:.3e}, max|F| = {scale:.3e}")
    assert worst <= 1e-9 * scale + 1e-9


@pytest.mark.parametrize("nw,ni", SIZES)
def test_reference_hv_matches_central_differences_of_the_oracle(nw, ni):
    force, confs, ref = _case(nw, ni)
    o = Oracle(force)
    rng = np.random.default_rng(41 + nw + ni)
    forces = lambda x: o.execute(x, None)["forces"]
    worst = 0.0
    for conf in confs:
        for v in rng.normal(size=(2,) + conf.shape):
            hv = ref.hv(conf, v)
            fd = -(forces(conf + H_FD * v) - forces(conf - H_FD * v)) / (2 * H_FD)
            worst = max(worst, np.abs(hv - fd).max() / np.abs(hv).max())
    print(f"{nw}+{ni}: max|Hv - fd| / max|Hv| = {worst:.3e}")
    assert worst <= FD_BAR


@pytest.mark.parametrize("nw,ni", SIZES)
def test_reference_symmetry_and_translations(nw, ni):
    force, confs, ref = _case(nw, ni)
    n = confs.shape[1]
    hmax = max(np.abs(hr.Reference(_case(2, 1)[0]).hessian(c)).max() for c in _case(2, 1)[1])
    rng = np.random.default_rng(43 + nw + ni)
    for conf in confs:
        u, v = rng.normal(size=(2, n, 3))
        hu, hv = ref.hv(conf, u), ref.hv(conf, v)
        asym = abs(np.sum(u * hv) - np.sum(v * hu))
        print(f"{nw}+{ni}: |u.Hv - v.Hu| = {asym:.3e}, |u||Hv| = {np.linalg.norm(u) * np.linalg.norm(hv):.3e}")
        assert asym <= 1e-12 * np.linalg.norm(u) * np.linalg.norm(hv)
        for axis in range(3):
            t = np.zeros((n, 3))
            t[:, axis] = 1.0
            assert np.abs(ref.hv(conf, t)).max() <= 1e-9 * hmax
