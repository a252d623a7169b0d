"""Helper of the ESP tests (not a test): cf_compute_batch_esp and its VJP (include/chargeflux.h;
DESIGN.md "Batched, electrostatic potential") restated in plain numpy, one conformation at a time,
with the charge model (pieces q_a += c_a k (g(x) - ref)) of tests/dipole_reference.py:
  V_p = ke sum_a q_a / r_pa          a_i = ke sum_p V_bar_p / r_pi          L = sum_p V_bar_p V_p
  dL/d(base charge i) = a_i,  dL/dk += (sum_a c_a a_a) (g - ref),  dL/dref += -k sum_a c_a a_a
The 1/r sums run in np.longdouble.  S_p = ke sum_a |q_a| / r_pa and S_i = ke sum_p |V_bar_p| / r_pi
are the magnitude sums the fp64 round-off of V_p and a_i is measured against.
"""
import numpy as np

from tests import dipole_reference as dr

KE = 138.935456   # the library's default one_4pi_eps0 (kJ nm / mol / e^2)


def evaluate(force, conf, points, esp_bar=None, theta=None):
    """One conformation.  Returns dict(q (N,), V (M,), S_V (M,), a (N,), S_a (N,), L, grad (P,)); a
    None cotangent is zero; theta: the flat parameters (default: the force's own)."""
    x, r = np.asarray(conf, dtype=np.float64), np.asarray(points, dtype=np.float64)
    n = force.getNumParticles()
    th = dr.flat_parameters(force) if theta is None else np.asarray(theta, dtype=np.float64)
    vb = np.zeros(len(r)) if esp_bar is None else np.asarray(esp_bar, dtype=np.float64)
    terms = [(atoms, c, dr.geometry(kind, ga, x)[0], ik, ir) for atoms, c, kind, ga, ik, ir in dr.pieces(force)]
    q = th[:n].copy()
    for atoms, c, g, ik, ir in terms:
        for at, ca in zip(atoms, c):
            q[at] += ca * th[ik] * (g - th[ir])
    d = (r[:, None, :] - x[None, :, :]).astype(np.longdouble)
    inv = 1 / np.sqrt((d * d).sum(axis=2))                       # (M, N) longdouble
    V, S_V = KE * (inv @ q), KE * (inv @ np.abs(q))
    a, S_a = KE * (vb @ inv), KE * (np.abs(vb) @ inv)
    a64 = a.astype(np.float64)
    grad = np.zeros(len(th))
    grad[:n] = a64
    for atoms, c, g, ik, ir in terms:
        ca_a = sum(ca * a64[at] for at, ca in zip(atoms, c))
        grad[ik] += ca_a * (g - th[ir])
        grad[ir] += -th[ik] * ca_a
    f64 = lambda v: v.astype(np.float64)
    return {"q": q, "V": f64(V), "S_V": f64(S_V), "a": a64, "S_a": f64(S_a), "L": float(vb @ V), "grad": grad}


def evaluate_batch(force, confs, points, esp_bar=None):
    """The same over (B,N,3) and (B,M,3): dict of stacked q, V, S_V, a, S_a, grad."""
    res = [evaluate(force, confs[b], points[b], None if esp_bar is None else esp_bar[b]) for b in range(len(confs))]
    return {key: np.stack([r[key] for r in res]) for key in ("q", "V", "S_V", "a", "S_a", "grad")}
