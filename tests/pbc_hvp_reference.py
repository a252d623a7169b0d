"""Helper of the periodic Hessian-vector tests (not a test): the periodic forces of one conformation
and box restated in plain numpy (include/chargeflux.h, cf_compute_batch_periodic: flux charges by
minimum image, erfc pairs and LJ within the cutoff, the erf correction of excluded pairs, the self
term, the exact half-space k-sum with k from the box diagonals, the chain rule), written so that the
positions may be COMPLEX, tests/hvp_reference.py's approach:

    H v = -D_v F = -Im F(x + i h v) / h,      h = 1e-30

  - minimum-image shifts, the cutoff test and the coordinate wrap are decided on the real parts (they
    are piecewise constant: the derivative is the one at fixed pair set and image);
  - the phases are cos and sin of complex arguments (the step's imaginary unit is not the phase's);
  - erfc(z) = erfc(Re z) - i Im z (2 / sqrt(pi)) exp(-(Re z)^2), exact at first order in Im z.
It shares no closed-form Hessian with the code under test.
"""
import math

import numpy as np

from tests.dipole_reference import geometry, pieces

KE = 138.935456   # the library's default one_4pi_eps0 (kJ nm / mol / e^2)
C = 2.0 / math.sqrt(math.pi)
_erfc = np.vectorize(math.erfc, otypes=[np.float64])


def erfc(z):
    z = np.asarray(z)
    re = _erfc(z.real)
    return re - 1j * z.imag * C * np.exp(-z.real ** 2) if np.iscomplexobj(z) else re


def min_image(d, box):
    """ReferenceForce::getDeltaRPeriodic on difference vectors (..., 3); rows of box: a, b, c."""
    d = d - np.floor(d[..., 2:3].real / box[2, 2] + 0.5) * box[2]
    d = d - np.floor(d[..., 1:2].real / box[1, 1] + 0.5) * box[1]
    return d - np.floor(d[..., 0:1].real / box[0, 0] + 0.5) * box[0]


class Reference:
    """One force's topology and Ewald parameters (alpha, kmax: the oracle's ewald()), read once."""

    def __init__(self, force, alpha, kmax, ke=KE):
        a = force.arrays()
        self.n = len(a["charges"])
        self.half_sigma = 0.5 * a["sigmas"]
        self.two_sqrt_eps = 2.0 * np.sqrt(a["epsilons"])
        self.ke, self.alpha, self.cutoff = ke, alpha, force.getCutoffDistance()
        self.pieces = pieces(force)
        self.theta = np.concatenate([a["charges"], a["fbond_par"].ravel(), a["fangle_par"].ravel(),
                                     a["fwater_par"].ravel()])
        self.excl = np.zeros((self.n, self.n), dtype=bool)
        for i, j in a["exceptions"]:
            self.excl[i, j] = self.excl[j, i] = True
        KX, KY, KZ = kmax
        self.kint = np.array([(0, 0, z) for z in range(1, KZ)]
                             + [(0, y, z) for y in range(1, KY) for z in range(1 - KZ, KZ)]
                             + [(x, y, z) for x in range(1, KX) for y in range(1 - KY, KY) for z in range(1 - KZ, KZ)],
                             dtype=np.float64).reshape(-1, 3)

    def forces(self, x, box):
        """F (N,3) at positions x (N,3), real or complex, in the box (3,3) (rows a, b, c)."""
        x = np.asarray(x)
        box = np.asarray(box, dtype=np.float64)
        n, ke, al = self.n, self.ke, self.alpha
        q = self.theta[:n].astype(x.dtype)
        dqdx = np.zeros((n, n, 3), dtype=x.dtype)          # [a][b]: dq_a / dx_b
        for atoms, c, kind, ga, ik, ir in self.pieces:
            xs = np.stack([x[ga[1]] + min_image(x[g] - x[ga[1]], box) for g in ga])   # images about ga[1]
            g, dg = geometry(kind, tuple(range(len(ga))), xs)
            k, ref = self.theta[ik], self.theta[ir]
            for at, ca in zip(atoms, c):
                q[at] = q[at] + ca * k * (g - ref)
                for b, gb in dg.items():
                    dqdx[at, ga[b]] = dqdx[at, ga[b]] + ca * k * gb
        d = min_image(x[:, None, :] - x[None, :, :], box)   # d[i][j] = x_i - x_j
        r2 = np.einsum("ijk,ijk->ij", d, d)                 # no conjugation
        off = ~np.eye(n, dtype=bool)
        near = off & ~self.excl & (r2.real <= self.cutoff ** 2)
        use = near | self.excl
        r = np.sqrt(np.where(use, r2, 1.0))
        ar = al * r
        ee = C * ar * np.exp(-ar * ar)
        p = np.where(self.excl, erfc(ar) - 1.0, erfc(ar))  # P = phi r: -erf or erfc
        sig = (self.half_sigma[:, None] + self.half_sigma[None, :]) / r
        s6 = (sig * sig) ** 3
        es6 = s6 * self.two_sqrt_eps[:, None] * self.two_sqrt_eps[None, :]
        cq = ke * q[:, None] * q[None, :] / r
        s = np.where(use, (np.where(near, es6 * (12.0 * s6 - 6.0), 0.0) + cq * (p + ee)) / (r * r), 0.0)
        f = np.einsum("ij,ijk->ik", s, d)
        g = np.where(use, ke * q[None, :] * p / r, 0.0).sum(axis=1) - 2.0 * ke * al / math.sqrt(math.pi) * q
        # reciprocal part: k from the box diagonals, coordinates wrapped by them
        L = np.diag(box)
        kv = self.kint * (2.0 * math.pi / L)
        th = (x - np.floor(x.real / L) * L) @ kv.T         # [i][k]
        co, si = np.cos(th), np.sin(th)
        k2 = (kv * kv).sum(axis=1)
        ck = 4.0 * math.pi * ke / np.prod(L) * np.exp(-k2 / (4.0 * al * al)) / k2
        ax, ay = 2.0 * ck * (q @ co), 2.0 * ck * (q @ si)  # A = 2 c_k S
        f = f + q[:, None] * ((ax * si - ay * co) @ kv)
        g = g + (ax * co + ay * si).sum(axis=1)
        return f - np.einsum("a,abk->bk", g, dqdx)

    def hv(self, x, box, v, h=1e-30):
        """H(x; box) v (N,3) by the complex step."""
        return -self.forces(np.asarray(x, dtype=np.float64) + 1j * h * np.asarray(v, dtype=np.float64), box).imag / h
