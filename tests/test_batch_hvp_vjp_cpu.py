"""CPU tests of the yardstick of cf_compute_batch_hvp_vjp (tests/hvp_vjp_reference.py) on the clusters
(2, 1) and (21, 7), to a tenth of the GPU bar per parameter group (max|a - b| <= 1e-10 max|a| + 1e-10):
the central differences at STEP and 2 STEP agree, and the base-charge rows equal sum_k g^uv written
directly from the closed form of include/chargeflux.h.  A null handle is rejected without a device.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from openmmcoul import _cabi
from tests import hvp_reference as hr
from tests import hvp_vjp_reference as hvr
from tests.dipole_reference import geometry
from tests.test_gpu_batch_vjp import _cluster, _conformations, _counts

REL = ABS = 1e-10


def test_null_handles_are_rejected():
    lib = _cabi.load_library()
    a = np.full((1, 1, 3, 3), 5.0)
    dp, vp = a.ctypes.data_as(C.POINTER(C.c_double)), C.c_void_p(a.ctypes.data)
    for rc in (lib.cf_compute_batch_hvp_vjp(None, 1, vp, 1, vp, vp, vp),
               lib.cf_compute_batch_hvp_vjp_host(None, 1, dp, 1, dp, dp, dp)):
        assert rc == _cabi.CF_ERR_INVALID and b"null" in lib.cf_last_error()
    assert (a == 5.0).all()


@functools.lru_cache(maxsize=None)
def _case(nw, ni):
    system, force, pos = _cluster(nw, ni)
    ref = hr.Reference(force)
    x = _conformations(pos, 177 + nw + ni)[0]
    vecs, ubar = np.random.default_rng(5 + nw + ni).normal(size=(2, 2) + x.shape)
    return force, ref, x, vecs, ubar, hvr.grad_rows(ref, x, vecs, ubar)


_close = functools.partial(hvr.check_groups, rel=REL, ab=ABS)


@pytest.mark.parametrize("nw,ni", [(2, 1), (21, 7)])
def test_the_two_steps_agree(nw, ni):
    force, ref, x, vecs, ubar, rows = _case(nw, ni)
    _close(f"{nw}+{ni}", rows, hvr.grad_rows(ref, x, vecs, ubar, 2 * hvr.STEP), _counts(force))


@pytest.mark.parametrize("nw,ni", [(2, 1), (21, 7)])
def test_base_charge_rows_equal_the_closed_form(nw, ni):
    force, ref, x, vecs, ubar, rows = _case(nw, ni)
    n, h = ref.n, 1e-30
    for k in range(len(vecs)):
        u, v = ubar[k], vecs[k]
        q, qu, qv, quv = ref.base.copy(), np.zeros(n), np.zeros(n), np.zeros(n)
        for atoms, c, kind, ga, ik, ir in ref.pieces:
            g, dg = geometry(kind, ga, x + 1j * h * v)            # gamma and its gradient, complex step along v
            gu = sum(gb @ u[b] for b, gb in dg.items())           # gamma^u (real part), gamma^uv (imaginary / h)
            for at, ca in zip(atoms, c):
                kk = ca * ref.theta[ik]
                q[at] += kk * (g.real - ref.theta[ir])
                qu[at] += kk * gu.real
                qv[at] += kk * g.imag / h
                quv[at] += kk * gu.imag / h
        d = x[None] - x[:, None]                                  # d[i][j] = x_j - x_i
        wu, wv = u[None] - u[:, None], v[None] - v[:, None]
        r = np.where(ref.mask, np.sqrt((d * d).sum(-1)), 1.0)
        du, dv, uv = (d * wu).sum(-1), (d * wv).sum(-1), (wu * wv).sum(-1)
        guv = ref.ke * np.where(ref.mask, quv[None] / r - (qu[None] * dv + qv[None] * du + q[None] * uv) / r**3
                                + 3 * q[None] * du * dv / r**5, 0.0).sum(1)
        _close(f"{nw}+{ni} row {k}", rows[k, :n], guv, (n,))
