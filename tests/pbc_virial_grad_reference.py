"""Helper of the virial parameter-gradient tests (not a test): L = W_bar : virial of one frame by ONE
complex step of tests/pbc_virial_reference.Reference along the strain T = (W_bar + W_bar^T) / 2,
    L(theta) = -Im E(x (I + i h T), box (I + i h T); theta) / h,      h = 1e-30, per energy part,
and its parameter gradients by differences of that L, per part ({part: (len(params),)}):
  - base charges and flux parameters (ref.theta): L is exactly quadratic in each parameter alone, so a
    central difference has no truncation error (step 1e-2, as test_gpu_batch_periodic_vjp.py);
  - LJ sigma / epsilon: the Richardson-extrapolated central differences (4 D(h/2) - D(h)) / 3 with
    tests/lj_reference.richardson_fd's step rule.
The parts cancel, so errors are measured against G = sum over the parts of the part's largest absolute
entry (`scale`).  It shares no closed-form derivative with the code under test.
"""
import copy

import numpy as np

from tests.pbc_virial_reference import PARTS

H_STRAIN = 1e-30
H_FD = 1e-2


def loss_parts(ref, x, box, w_bar):
    """{part: L_part} of one frame."""
    t = 0.5 * (np.asarray(w_bar) + np.asarray(w_bar).T)
    m = np.eye(3) + 1j * H_STRAIN * t
    return {p: -e.imag / H_STRAIN for p, e in ref.energy_parts(x @ m, box @ m).items()}


def _moved(ref, p, delta, lj):
    """A copy of ref with theta_p moved, or (lj) the LJ parameter p: sigma_p for p < N, else eps_{p-N}
    (Reference keeps sigma / 2 and 2 sqrt eps)."""
    r = copy.copy(ref)
    r.theta, r.half_sigma, r.two_sqrt_eps = ref.theta.copy(), ref.half_sigma.copy(), ref.two_sqrt_eps.copy()
    if not lj:
        r.theta[p] += delta
    elif p < ref.n:
        r.half_sigma[p] += 0.5 * delta
    else:
        r.two_sqrt_eps[p - ref.n] = 2.0 * np.sqrt((0.5 * ref.two_sqrt_eps[p - ref.n]) ** 2 + delta)
    return r


def _difference(ref, x, box, w_bar, p, step, lj=False):
    lp, lm = (loss_parts(_moved(ref, p, s, lj), x, box, w_bar) for s in (step, -step))
    return {part: (lp[part] - lm[part]) / (2 * step) for part in PARTS}


def theta_gradient(ref, x, box, w_bar, params, step=H_FD):
    """{part: dL_part/dtheta_p over params} by central differences."""
    cols = [_difference(ref, x, box, w_bar, p, step) for p in params]
    return {part: np.array([c[part] for c in cols]) for part in PARTS}


def lj_gradient(ref, x, box, w_bar, params):
    """{part: dL_part/d(sigma, eps)_p over params (flat: sigma_i at i, eps_i at N + i)}."""
    cols = []
    for p in params:
        value = 2.0 * ref.half_sigma[p] if p < ref.n else (0.5 * ref.two_sqrt_eps[p - ref.n]) ** 2
        h = 1e-3 * (value if value != 0.0 else 2.0 * ref.half_sigma.max())
        d1, d2 = (_difference(ref, x, box, w_bar, p, s, lj=True) for s in (h, 0.5 * h))
        cols.append({part: (4 * d2[part] - d1[part]) / 3 for part in PARTS})
    return {part: np.array([c[part] for c in cols]) for part in PARTS}


def total(parts):
    return sum(parts[p] for p in PARTS)


def scale(*gradients):
    """G over any number of per-part gradient dicts (e.g. the frames of a batch)."""
    return sum(max(np.abs(g[p]).max() for g in gradients) for p in PARTS)


def strided(counts, stride=8, offset=0):
    """Flat indices offset, offset + stride, ... and both ends of every non-empty group of `counts`."""
    edges = np.cumsum((0,) + tuple(counts))
    ends = [int(e) for lo, hi in zip(edges[:-1], edges[1:]) if hi > lo for e in (lo, hi - 1)]
    return sorted(set(range(offset, int(edges[-1]), stride)) | set(ends))
