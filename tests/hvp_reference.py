"""Helper of the Hessian-vector tests (not a test): the non-periodic forces of one conformation
restated in plain numpy (flux charges, pair forces, chain rule; include/chargeflux.h,
cf_compute_batch), written so that the positions may be COMPLEX: sqrt(d @ d) without conjugation,
np.arccos, no abs or norm.  The Hessian-vector product then needs no second derivative written
down twice:

    H v = -D_v F = -Im F(x + i h v) / h,      h = 1e-30

The complex step has no subtraction, so it is exact to round-off whatever h: the yardstick of
cf_compute_batch_hvp shares no closed-form Hessian with the code under test.

    q_a   = base_a + sum_pieces c_a k (g(x) - ref)            (tests/dipole_reference.py: pieces)
    E     = sum_{i<j, not excluded} [4 sqrt(eps_i eps_j) s6 (s6 - 1) + ke q_i q_j / r],
            s6 = ((sigma_i + sigma_j) / 2 r)^6
    F_i   = -dE/dx_i at fixed q  -  sum_a g_a dq_a/dx_i,      g_a = ke sum_j q_j / r_aj
"""
import numpy as np

from tests.dipole_reference import geometry, pieces

KE = 138.935456   # the library's default one_4pi_eps0 (kJ nm / mol / e^2)


class Reference:
    """The topology of one force, read once; forces(x) and hv(x, v) of a conformation."""

    def __init__(self, force, ke=KE):
        a = force.arrays()
        self.n = len(a["charges"])
        self.base = a["charges"].astype(np.float64)
        self.half_sigma = 0.5 * a["sigmas"]
        self.two_sqrt_eps = 2.0 * np.sqrt(a["epsilons"])
        self.ke = ke
        self.pieces = [(atoms, c, kind, ga, a_k, a_r) for atoms, c, kind, ga, a_k, a_r in pieces(force)]
        self.theta = np.concatenate([a["charges"], a["fbond_par"].ravel(), a["fangle_par"].ravel(),
                                     a["fwater_par"].ravel()])
        mask = ~np.eye(self.n, dtype=bool)
        for i, j in a["exceptions"]:
            mask[i, j] = mask[j, i] = False
        self.mask = mask

    def forces(self, x):
        """F (N,3) at positions x (N,3), real or complex."""
        x = np.asarray(x)
        n, ke = self.n, self.ke
        q = self.base.astype(x.dtype)
        dqdx = np.zeros((n, n, 3), dtype=x.dtype)          # [a][b]: dq_a / dx_b
        for atoms, c, kind, ga, ik, ir in self.pieces:
            g, dg = geometry(kind, ga, x)
            k, ref = self.theta[ik], self.theta[ir]
            for at, ca in zip(atoms, c):
                q[at] = q[at] + ca * k * (g - ref)
                for b, gb in dg.items():
                    dqdx[at, b] = dqdx[at, b] + ca * k * gb
        d = x[None, :, :] - x[:, None, :]                   # d[i][j] = x_j - x_i
        r2 = np.einsum("ijk,ijk->ij", d, d)                 # no conjugation
        r2 = np.where(self.mask, r2, 1.0)
        inv_r = 1.0 / np.sqrt(r2)
        sig = self.half_sigma[:, None] + self.half_sigma[None, :]
        s2 = sig * inv_r * sig * inv_r
        s6 = s2 * s2 * s2
        es6 = s6 * self.two_sqrt_eps[:, None] * self.two_sqrt_eps[None, :]
        qq = ke * q[:, None] * q[None, :] * inv_r
        s = np.where(self.mask, (es6 * (12.0 * s6 - 6.0) + qq) * inv_r * inv_r, 0.0)
        f_pair = -np.einsum("ij,ijk->ik", s, d)
        g = np.where(self.mask, ke * q[None, :] * inv_r, 0.0).sum(axis=1)
        return f_pair - np.einsum("a,abk->bk", g, dqdx)

    def hv(self, x, v, h=1e-30):
        """H(x) v (N,3) by the complex step."""
        return -self.forces(np.asarray(x, dtype=np.float64) + 1j * h * np.asarray(v, dtype=np.float64)).imag / h

    def hessian(self, x):
        """The full (3N,3N) Hessian, column by column; not symmetrised."""
        n3 = 3 * self.n
        cols = [self.hv(x, e.reshape(self.n, 3)).ravel() for e in np.eye(n3)]
        return np.stack(cols, axis=1)
