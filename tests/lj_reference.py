"""Helper of the LJ-gradient tests (not a test): the closed form of cf_compute_batch_lj_vjp
(include/chargeflux.h; DESIGN.md "Batched, LJ parameter gradients") restated in numpy, and the
Richardson-extrapolated central differences of the oracle it is checked against.

Per conformation, with cotangents e_bar (scalar) and v = F_bar (N,3), L = e_bar E + sum v_i . F_i.
The kernels store lj_i = (sigma_i / 2, 2 sqrt(eps_i)); a pair carries U = e4 s6 (s6 - 1) with
A = lj_i.x + lj_j.x, e4 = lj_i.y lj_j.y, s6 = (A / r)^6, over every non-excluded pair (periodic:
minimum image, r^2 <= cutoff^2).  An atom with eps = 0 gets exactly 0 for both gradients.

L is not polynomial in sigma: plain central differences at h = 1e-3 sigma miss by ~1e-6 relative.
The extrapolated form (4 D(h/2) - D(h)) / 3 removes the h^2 term and is good to ~1e-11.
"""
import copy

import numpy as np

from oracle import Oracle


def min_image(d, box):
    """ReferenceForce::getDeltaRPeriodic on an array of difference vectors (rows of box: a, b, c;
    reduced triclinic form, c, b, a order)."""
    d = d.copy()
    d -= np.floor(d[..., 2:3] / box[2, 2] + 0.5) * box[2]
    d -= np.floor(d[..., 1:2] / box[1, 1] + 0.5) * box[1]
    d -= np.floor(d[..., 0:1] / box[0, 0] + 0.5) * box[0]
    return d


def _excluded(force):
    n = force.getNumParticles()
    skip = np.eye(n, dtype=bool)
    for k in range(force.getNumExceptions()):
        i, j = force.getExceptionParameters(k)[:2]
        skip[i, j] = skip[j, i] = True
    return skip


def pair_gap_to_cutoff(force, conf, box):
    """min | r - cutoff | over the non-excluded minimum-image pairs (inf if there are none)."""
    r = np.linalg.norm(min_image(conf[:, None, :] - conf[None, :, :], np.asarray(box)), axis=2)
    gap = np.abs(r - force.getCutoffDistance())[~_excluded(force)]
    return gap.min() if gap.size else np.inf


def closed_form(force, conf, box=None, e_bar=None, f_bar=None):
    """(dL/dsigma (N,), dL/deps (N,)) of one conformation; box: (3,3) for a periodic force, else None;
    a None cotangent is zero."""
    n = force.getNumParticles()
    a = force.arrays()
    ljx, ljy = 0.5 * a["sigmas"], 2.0 * np.sqrt(a["epsilons"])
    eb = 0.0 if e_bar is None else float(e_bar)
    v = np.zeros((n, 3)) if f_bar is None else np.asarray(f_bar, dtype=np.float64)
    skip = _excluded(force)
    pbc = force.usesPeriodicBoundaryConditions()
    rc2 = force.getCutoffDistance() ** 2
    gs, ge = np.zeros(n), np.zeros(n)
    dall = conf[:, None, :] - conf[None, :, :]          # [i, j] = x_i - x_j
    if pbc:
        dall = min_image(dall, np.asarray(box))
    for i in range(n):
        if ljy[i] == 0.0:
            continue
        gsi = tpi = 0.0
        for j in range(n):
            if skip[i, j] or ljy[j] == 0.0:
                continue
            d = dall[i, j]
            r2 = float(d @ d)
            if pbc and not r2 <= rc2:
                continue
            A = ljx[i] + ljx[j]
            a5r6 = A ** 5 / r2 ** 3
            s6 = a5r6 * A
            rr = float(d @ (v[i] - v[j])) / r2          # rdot / r
            gsi += ljy[i] * ljy[j] * a5r6 * (eb * (12 * s6 - 6) + (144 * s6 - 36) * rr)
            tpi += ljy[j] * (eb * s6 * (s6 - 1) + (12 * s6 * s6 - 6 * s6) * rr)
        gs[i] = 0.5 * gsi
        ge[i] = 2.0 * tpi / ljy[i]
    return gs, ge


def active_parameters(force):
    """Flat indices (sigma_i: i, eps_i: N + i) of the LJ parameters of the atoms with eps > 0."""
    n = force.getNumParticles()
    on = [i for i in range(n) if force._eps[i] > 0.0]
    return on + [n + i for i in on]


def _loss(res, e_bar, f_bar):
    v = 0.0
    if e_bar is not None:
        v += float(e_bar) * res["energy"]
    if f_bar is not None:
        v += float(np.sum(f_bar * res["forces"]))
    return v


def richardson_fd(force, default_box, confs, boxes, cots, params):
    """{set: (len(confs), len(params))}: (4 D(h/2) - D(h)) / 3 of the oracle, D the central difference,
    h = 1e-3 * value, on a deep copy of the force with _sigma[i] / _eps[i] moved (flat index p < N:
    sigma_p, else eps_{p-N}).  A sigma of 0 has no scale of its own: its h is 1e-3 of the largest
    sigma of the force.  confs: list of (N,3); boxes: list of (3,3) or None; cots: {set: (e_bar
    (B,) or None, f_bar (B,N,3) or None)}.  One oracle per moved force, shared by conformations and sets."""
    n = force.getNumParticles()
    out = {s: np.zeros((len(confs), len(params))) for s in cots}
    for col, p in enumerate(params):
        store, i = ("_sigma", p) if p < n else ("_eps", p - n)
        value = getattr(force, store)[i]
        h = 1e-3 * (value if value != 0.0 else max(force._sigma))
        d = {}
        for step in (h, 0.5 * h):
            res = []
            for sign in (1.0, -1.0):
                f = copy.deepcopy(force)
                getattr(f, store)[i] = value + sign * step
                o = Oracle(f, default_box)
                res.append([o.execute(confs[b], None if boxes is None else boxes[b]) for b in range(len(confs))])
            for s, (eb, fb) in cots.items():
                for b in range(len(confs)):
                    lp = _loss(res[0][b], None if eb is None else eb[b], None if fb is None else fb[b])
                    lm = _loss(res[1][b], None if eb is None else eb[b], None if fb is None else fb[b])
                    d[(s, b, step)] = (lp - lm) / (2 * step)
        for s in cots:
            for b in range(len(confs)):
                out[s][b, col] = (4 * d[(s, b, 0.5 * h)] - d[(s, b, h)]) / 3
    return out
