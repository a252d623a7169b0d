"""Helper of the dipole / polar-tensor tests (not a test): cf_compute_batch_dipole and its VJP
(include/chargeflux.h; DESIGN.md "Batched, dipoles and polar tensors") restated in plain numpy from
the formulas, one conformation at a time.

Every flux term is a sum of elementary pieces  q_a += c_a k (g(x) - ref)  over the piece's atoms:
  bond (p1, p2; k, b)                 g = |x2 - x1|, c = (1, -1)
  angle (p1, p2, p3; k, theta0)       g = the angle at p2, c = (1, -2, 1)
  water (O, H1, H2; k1, k2, kub, b0, ub0)
      k1 (r_OH1 - b0)  into H1, k1 (r_OH2 - b0) into H2,
      k2 (r_OH2 - b0)  into H1, k2 (r_OH1 - b0) into H2,
      kub (r_HH - ub0) into H1 and H2, and the oxygen takes minus what the hydrogens get.
With q the charges after flux:
  mu_al        = sum_a q_a x_a,al                          (about the coordinate origin)
  P[b][al][be] = q_b delta_al,be + sum_pieces k (sum_a c_a x_a,al) (grad_b g)_be
and for L = mu_bar . mu + sum_b P_bar_b : P_b, with a_i = mu_bar . x_i + tr P_bar_i and
w = sum_a c_a x_a:
  dL/d(base charge i) = a_i
  dL/dk   += (sum_a c_a a_a) (g - ref) + sum_b w^T P_bar_b grad_b g
  dL/dref += -k sum_a c_a a_a
The flat parameter vector is the row layout of cf_get_param_counts: base charges [N], bonds (k, b),
angles (k, theta0), waters (k1, k2, kub, b0, ub0).
"""
import numpy as np


def flat_parameters(force):
    a = force.arrays()
    return np.concatenate([a["charges"], a["fbond_par"].ravel(), a["fangle_par"].ravel(), a["fwater_par"].ravel()])


def pieces(force):
    """[(atoms, c, kind, geometry atoms, flat index of k, flat index of ref)]; kind 'r' (distance
    between the two geometry atoms) or 'theta' (angle at the middle one of three)."""
    a = force.arrays()
    n = len(a["charges"])
    out = []
    off = n
    for t, (p1, p2) in enumerate(a["fbond_idx"]):
        out.append(((p1, p2), (1.0, -1.0), "r", (p1, p2), off + 2 * t, off + 2 * t + 1))
    off += 2 * len(a["fbond_idx"])
    for t, (p1, p2, p3) in enumerate(a["fangle_idx"]):
        out.append(((p1, p2, p3), (1.0, -2.0, 1.0), "theta", (p1, p2, p3), off + 2 * t, off + 2 * t + 1))
    off += 2 * len(a["fangle_idx"])
    for t, (o, h1, h2) in enumerate(a["fwater_idx"]):
        k1, k2, kub, b0, ub0 = (off + 5 * t + j for j in range(5))
        atoms = (o, h1, h2)
        to_h1, to_h2 = (-1.0, 1.0, 0.0), (-1.0, 0.0, 1.0)
        out.append((atoms, to_h1, "r", (o, h1), k1, b0))
        out.append((atoms, to_h2, "r", (o, h2), k1, b0))
        out.append((atoms, to_h1, "r", (o, h2), k2, b0))
        out.append((atoms, to_h2, "r", (o, h1), k2, b0))
        out.append((atoms, (-2.0, 1.0, 1.0), "r", (h1, h2), kub, ub0))
    return [(tuple(int(i) for i in at), c, kind, tuple(int(i) for i in ga), int(ik), int(ir))
            for at, c, kind, ga, ik, ir in out]


def geometry(kind, ga, x):
    """(g, {atom: grad_atom g (3,)}) of one piece's geometry."""
    if kind == "r":
        i, j = ga
        d = x[j] - x[i]
        r = np.sqrt(d @ d)
        return r, {i: -d / r, j: d / r}
    i, j, k = ga
    d1, d3 = x[i] - x[j], x[k] - x[j]
    r1, r3 = np.sqrt(d1 @ d1), np.sqrt(d3 @ d3)
    e1, e3 = d1 / r1, d3 / r3
    cos = e1 @ e3
    sin = np.sqrt(1.0 - cos * cos)
    g1 = (cos * e1 - e3) / (r1 * sin)
    g3 = (cos * e3 - e1) / (r3 * sin)
    return np.arccos(cos), {i: g1, j: -g1 - g3, k: g3}


def evaluate(force, conf, mu_bar=None, p_bar=None, theta=None):
    """One conformation.  Returns dict(q (N,), mu (3,), P (N,3,3), L, grad (P,)); a None cotangent is
    zero; theta: the flat parameters (default: the force's own)."""
    x = np.asarray(conf, dtype=np.float64)
    n = force.getNumParticles()
    th = flat_parameters(force) if theta is None else np.asarray(theta, dtype=np.float64)
    mb = np.zeros(3) if mu_bar is None else np.asarray(mu_bar, dtype=np.float64)
    pb = np.zeros((n, 3, 3)) if p_bar is None else np.asarray(p_bar, dtype=np.float64)
    a = x @ mb + np.trace(pb, axis1=1, axis2=2)
    q = th[:n].copy()
    flux = np.zeros((n, 3, 3))
    grad = np.zeros(len(th))
    grad[:n] = a
    for atoms, c, kind, ga, ik, ir in pieces(force):
        g, dg = geometry(kind, ga, x)
        k, ref = th[ik], th[ir]
        w = sum(ca * x[at] for at, ca in zip(atoms, c))
        ca_a = sum(ca * a[at] for at, ca in zip(atoms, c))
        for at, ca in zip(atoms, c):
            q[at] += ca * k * (g - ref)
        bil = 0.0
        for b, gb in dg.items():
            flux[b] += k * np.outer(w, gb)
            bil += w @ pb[b] @ gb
        grad[ik] += ca_a * (g - ref) + bil
        grad[ir] += -k * ca_a
    mu = q @ x
    P = flux + q[:, None, None] * np.eye(3)
    return {"q": q, "mu": mu, "P": P, "L": float(mb @ mu + np.sum(pb * P)), "grad": grad}


def evaluate_batch(force, confs, mu_bar=None, p_bar=None):
    """The same over (B,N,3): dict of stacked q (B,N), mu (B,3), P (B,N,3,3), grad (B,P)."""
    res = [evaluate(force, confs[b], None if mu_bar is None else mu_bar[b], None if p_bar is None else p_bar[b])
           for b in range(len(confs))]
    return {key: np.stack([r[key] for r in res]) for key in ("q", "mu", "P", "grad")}
