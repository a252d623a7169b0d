"""Helper of the cf_compute_batch_hvp_vjp tests (not a test): the parameter gradient of
L(theta) = sum_k u_k . H(x; theta) v_k by central differences of the complex-step products of
tests/hvp_reference.py.  The charges are affine in every single parameter and the energy is quadratic
in the charges, so L is a quadratic polynomial along any line that keeps q affine -- one parameter,
or a direction touching only (base charges, k-type) or only ref-type parameters -- and the central
difference is exact up to round-off whatever the step.  STEP = 1/8, of the order of the parameters
(0.1 .. 2) and exact in binary; tests/test_batch_hvp_vjp_cpu.py checks it against 2 STEP.
"""
import copy

import numpy as np

STEP = 0.125


def loss_rows(ref, theta, x, vecs, ubar):
    """(K,): u_k . H(x; theta) v_k, theta in cf_get_param_counts order (its head is the base charges)."""
    r = copy.copy(ref)
    r.theta, r.base = theta, theta[:ref.n].copy()
    return np.array([np.sum(ubar[k] * r.hv(x, vecs[k])) for k in range(len(vecs))])


def directional(ref, x, vecs, ubar, dtheta, h=STEP):
    """(K,): d/dt of loss_rows at theta + t dtheta."""
    return (loss_rows(ref, ref.theta + h * dtheta, x, vecs, ubar)
            - loss_rows(ref, ref.theta - h * dtheta, x, vecs, ubar)) / (2 * h)


def grad_rows(ref, x, vecs, ubar, h=STEP):
    """(K,P): every direction's own gradient row, parameter by parameter."""
    return np.stack([directional(ref, x, vecs, ubar, e, h) for e in np.eye(len(ref.theta))], axis=1)


def seeded_directions(ref, seed, count):
    """count N(0,1) directions over the base charges and k-type parameters, then count over the
    ref-type ones (b, theta0, b0, ub0): (2 count, P)."""
    is_ref = np.zeros(len(ref.theta), dtype=bool)
    is_ref[[ir for *_, ir in ref.pieces]] = True
    d = np.random.default_rng(seed).normal(size=(2 * count, len(ref.theta)))
    d[:count, is_ref] = 0.0
    d[count:, ~is_ref] = 0.0
    return d


def check_groups(tag, got, ref, counts, rel, ab):
    """max|got - ref| <= rel max|ref| + ab per parameter group (charges, bonds, angles, waters), printed."""
    assert got.shape == ref.shape and np.isfinite(got).all()
    for name, lo, hi in zip(("charges", "bonds", "angles", "waters"), np.cumsum((0,) + counts[:-1]), np.cumsum(counts)):
        if hi > lo:
            err, scale = np.abs(got[..., lo:hi] - ref[..., lo:hi]).max(), np.abs(ref[..., lo:hi]).max()
            print(f"{tag} {name}: max|got - ref| = {err:.3e}, max|ref| = {scale:.3e}, ratio = {err / max(scale, 1e-300):.3e}")
            assert err <= rel * scale + ab, (tag, name, err, scale)
