"""Helper of the periodic virial tests (not a test): the energy of one frame of
cf_compute_batch_periodic (include/chargeflux.h) restated in plain numpy IN PARTS -- real-space pairs
with LJ, the erf correction of excluded pairs, the self term, the reciprocal sum -- with the charges
from the flux pieces of tests/dipole_reference.py, written so that the positions AND the box may be
COMPLEX (tests/pbc_hvp_reference.py's approach):

    virial = -dE/d eps = -Im E(x (I + i h e), box (I + i h e)) / h,    h = 1e-30, e the nine unit strains

  - minimum-image shifts, the cutoff test and the coordinate wrap are decided on the real parts (or on
    a given unstrained frame, `at=`): the derivative at fixed pair set and images;
  - the k-vectors follow the lattice, k = 2 pi n (box^-1)^T, the volume is det(box): for an
    orthorhombic box at e = 0 the forward call's 2 pi n / L and Lx Ly Lz;
  - erfc is extended as in pbc_hvp_reference.
It shares no closed-form virial with the code under test.
"""
import math

import numpy as np

from tests.dipole_reference import geometry
from tests.pbc_hvp_reference import Reference as _Topology
from tests.pbc_hvp_reference import erfc

PARTS = ("pair", "excl", "self", "recip")


def _shifts(d, box):
    """Integer lattice shifts (..., 3) of ReferenceForce::getDeltaRPeriodic for real d and box."""
    nc = np.floor(d[..., 2] / box[2, 2] + 0.5)
    d = d - nc[..., None] * box[2]
    nb = np.floor(d[..., 1] / box[1, 1] + 0.5)
    d = d - nb[..., None] * box[1]
    return np.stack([np.floor(d[..., 0] / box[0, 0] + 0.5), nb, nc], axis=-1)


class Reference(_Topology):
    def energy_parts(self, x, box, at=None):
        """{part: E_part} at positions x (N,3) in the box (3,3) (rows a, b, c), real or complex; every
        geometric decision on the real frame `at` = (x0, box0) (default: the real parts)."""
        x, box = np.asarray(x), np.asarray(box)
        x0, box0 = (x.real, box.real) if at is None else at
        n, ke, al = self.n, self.ke, self.alpha
        image = lambda i, j: (x[i] - x[j]) - _shifts(x0[i] - x0[j], box0) @ box
        q = self.theta[:n].astype(np.result_type(x.dtype, box.dtype))
        for atoms, c, kind, ga, ik, ir in self.pieces:
            xs = np.stack([x[ga[1]] + image(g, ga[1]) for g in ga])   # images about ga[1]
            g, _ = geometry(kind, tuple(range(len(ga))), xs)
            for a, ca in zip(atoms, c):
                q[a] = q[a] + ca * self.theta[ik] * (g - self.theta[ir])
        idx = np.arange(n)
        d = image(idx[:, None], idx[None, :])
        d0 = (x0[:, None, :] - x0[None, :, :]) - _shifts(x0[:, None, :] - x0[None, :, :], box0) @ box0
        off = ~np.eye(n, dtype=bool)
        near = off & ~self.excl & ((d0 * d0).sum(axis=2) <= self.cutoff ** 2)
        r = np.sqrt(np.where(near | self.excl, np.einsum("ijk,ijk->ij", d, d), 1.0))   # no conjugation
        qq = ke * q[:, None] * q[None, :] / r
        s6 = ((self.half_sigma[:, None] + self.half_sigma[None, :]) / r) ** 6
        lj = s6 * self.two_sqrt_eps[:, None] * self.two_sqrt_eps[None, :] * (s6 - 1.0)
        out = {"pair": 0.5 * np.where(near, qq * erfc(al * r) + lj, 0.0).sum(),
               "excl": -0.5 * np.where(self.excl, qq * (1.0 - erfc(al * r)), 0.0).sum(),
               "self": -ke * al / math.sqrt(math.pi) * (q * q).sum()}
        kv = 2.0 * math.pi * self.kint @ np.linalg.inv(box).T
        th = (x - np.floor(x0 / np.diag(box0)) @ box) @ kv.T   # wrapped as the forward wraps (orthorhombic)
        k2 = (kv * kv).sum(axis=1)
        ck = 4.0 * math.pi * ke / np.linalg.det(box) * np.exp(-k2 / (4.0 * al * al)) / k2
        out["recip"] = (ck * ((q @ np.cos(th)) ** 2 + (q @ np.sin(th)) ** 2)).sum()
        return out

    def virial_parts(self, x, box, h=1e-30):
        """{part: (3,3) -dE_part/d eps} by the complex step, and their sum under 'total'."""
        x, box = np.asarray(x, dtype=np.float64), np.asarray(box, dtype=np.float64)
        out = {p: np.zeros((3, 3)) for p in PARTS}
        for a in range(3):
            for b in range(3):
                m = np.eye(3, dtype=np.complex128)
                m[a, b] += 1j * h
                for p, e in self.energy_parts(x @ m, box @ m).items():
                    out[p][a, b] = -e.imag / h
        out["total"] = sum(out[p] for p in PARTS)
        return out
