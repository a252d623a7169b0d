"""Helper of the cf_compute_batch_periodic_hvp_vjp tests (not a test): tests/pbc_hvp_reference.Reference
with a bound box, so that tests/hvp_vjp_reference's loss_rows, directional, grad_rows,
seeded_directions and check_groups work on it unchanged.  In a box too the charges are affine in every
single parameter and the self, pair and reciprocal energies are quadratic in the charges: L is a
quadratic polynomial along any single parameter and the central difference at STEP has no truncation
error (tests/test_batch_periodic_hvp_vjp_cpu.py checks it against 2 STEP).
"""
import numpy as np

from tests import pbc_hvp_reference as pr


class Reference(pr.Reference):
    def __init__(self, force, alpha, kmax, box, ke=pr.KE):
        super().__init__(force, alpha, kmax, ke)
        self.box = np.asarray(box, dtype=np.float64)

    def hv(self, x, v, h=1e-30):
        """H(x; box) v (N,3) by the complex step, the signature of tests/hvp_reference.Reference.hv."""
        return super().hv(x, self.box, v, h)
