"""GPU tests of the parameter gradients of the periodic batch (cf_compute_batch_periodic_vjp,
include/chargeflux.h; DESIGN.md "Batched, periodic, parameter gradients"): against central
differences of the oracle, terms with k = 0, linearity in the cotangents and the NULL cases, the
bitwise guarantees, isolation from the single-evaluation state and from the forward periodic batch,
parameter updates, the argument errors and the torch autograd layer (openmmcoul.fitting with boxes=).

Systems: the recipes of test_gpu_batch_periodic.py, re-stated here.  B = 3 conformations, each with
its own box: base positions + N(0, 0.003 nm), the default box scaled per axis by factors in
[0.95, 1.05] with the positions scaled along; in conformation 1 every fifth atom is moved by a whole
box vector (molecules split across images: a gradient that forgets the minimum image in the term
geometry fails there).  The triclinic system's conformations 0 and 1 are sheared within the reduced
form, conformation 2 is orthorhombic.

The scalar differentiated per conformation is L = e_bar E + q_bar . q + F_bar . F.  The pair set,
alpha and kmax do not depend on the parameters, so L is exactly quadratic in every single parameter
in the periodic case too and a central difference along one parameter has no truncation error, only
round-off ~ eps |L| / h: h = 1e-2 in the parameter's own unit.  That needs the pair set to be the
same for the oracle and the kernels: the tests assert (a condition on the inputs, not a tolerance)
that no non-excluded minimum-image pair of a checked conformation lies within 1e-9 nm of the cutoff.

Bar (every finite-difference comparison here):  max |grad - fd| <= 1e-9 max |grad| + 1e-9, the maxima
taken per system and cotangent set over the checked conformations (max |grad| over all of their
parameters).  Observed on MI355X (printed by the tests): see DESIGN.md.
"""
import copy
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import Oracle  # noqa: E402
from openmmcoul import ChargeFluxError, CoulForce, HipCalcCoulForceKernel, System, _cabi  # noqa: E402
from openmmcoul import testsystems as ts  # noqa: E402

B = 3
H_FD = 1e-2
REL, ABS = 1e-9, 1e-9
SETS = ("E", "q", "F", "EqF")
SYSTEMS = ["w1", "ions", "w22", "tric", "aniso", "w100"]
SAMPLED = ("aniso", "w100")    # 64 sampled parameters, conformation 0 only


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _ions():
    """6 ions (+-1 e, sigma 0.3 nm, eps 0.5 kJ/mol) on a jittered 0.3 nm lattice in a 0.9 nm box,
    cutoff 0.4: no flux terms; two exceptions, atoms 0-1 closer than the cutoff (0.3 nm) and atoms
    0-3 farther apart than it (0.52 nm), so the exclusion correction is applied with no cutoff test."""
    rng = np.random.default_rng(ts.SEED + 6)
    sites = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 1), (2, 2, 0), (0, 2, 2)], dtype=np.float64)
    pos = (sites + 0.5) * 0.3 + rng.uniform(-0.02, 0.02, size=(6, 3))
    force, system = CoulForce(), System()
    for i in range(6):
        force.addParticle(1.0 if i % 2 == 0 else -1.0, 0.3, 0.5)
        system.addParticle(22.99 if i % 2 == 0 else 35.45)
    force.addException(0, 1)
    force.addException(0, 3)
    force.setUsesPeriodicBoundaryConditions(True)
    force.setCutoffDistance(0.4)
    force.setEwaldErrorTolerance(1e-4)
    box = np.diag([0.9, 0.9, 0.9])
    system.setDefaultPeriodicBoxVectors(*box)
    system.addForce(force)
    return system, force, pos, box


def _aniso():
    """64 waters by water_box's recipe (4 x 4 x 4 lattice, +-0.02 nm jitter, every 10th molecule
    bond + angle) in a default box of 1.0 x 1.25 x 1.55 nm, cutoff 0.45: three different kmax."""
    rng = np.random.default_rng(ts.SEED + 64)
    L = np.array([1.0, 1.25, 1.55])
    idx = np.array([(i, j, k) for i in range(4) for j in range(4) for k in range(4)], dtype=np.float64)
    centres = (idx + 0.5) * (L / 4) + rng.uniform(-0.02, 0.02, size=(64, 3))
    pos = ts._water_geometry(rng, centres).reshape(-1, 3)
    force, system = CoulForce(), System()
    for w in range(64):
        for q, s, e, mass in ((ts.Q_O, ts.SIG_O, ts.EPS_O, 15.999), (ts.Q_H, 0.0, 0.0, 1.008), (ts.Q_H, 0.0, 0.0, 1.008)):
            force.addParticle(q, s, e)
            system.addParticle(mass)
    for w in range(64):
        ts.add_water(force, 3 * w, w % 10 == 9)
    force.setUsesPeriodicBoundaryConditions(True)
    force.setCutoffDistance(0.45)
    force.setEwaldErrorTolerance(1e-4)
    box = np.diag(L)
    system.setDefaultPeriodicBoxVectors(*box)
    system.addForce(force)
    return system, force, pos, box


def _system(name, seed=ts.SEED):
    if name == "w1":      # fewer atoms than a wave, every pair excluded: self, k-space, exclusions only
        return ts.water_box(1, cutoff=0.13, seed=seed)
    if name == "ions":
        return _ions()
    if name == "w22":     # across one wave; FluxWater mixed with bond and angle terms
        return ts.water_box(22, cutoff=0.39, every_bond_angle=2, seed=seed)
    if name == "w100":    # across a 256-entry j tile with a tail
        return ts.water_box(100, cutoff=0.64, seed=seed)
    if name == "aniso":
        return _aniso()
    if name == "tric":
        return ts.triclinic_water_box(27, cutoff=0.41, seed=seed)
    raise KeyError(name)


def _conformations(name, pos, box, seed, nconf=B):
    """(confs (nconf,N,3), boxes (nconf,3,3)).  Box b = the default box with column a scaled by
    s[b,a] in [0.95, 1.05] (per-axis scaling of a reduced box, positions scaled along).  The triclinic
    system also gets its own shears per conformation, within the reduced form, and its conformation
    2 is orthorhombic (molecules moved rigidly with their oxygen's fractional coordinates, so the
    lattice of centres follows the box).  Conformation 1: every fifth atom by a whole box vector."""
    rng = np.random.default_rng(seed)
    n = len(pos)
    confs = np.empty((nconf, n, 3))
    boxes = np.empty((nconf, 3, 3))
    for b in range(nconf):
        s = rng.uniform(0.95, 1.05, size=3)
        x = pos + rng.normal(0.0, 0.003, size=pos.shape)
        bb = box * s[None, :]
        x = x * s[None, :]
        if name == "tric":
            shear = np.zeros(3) if b == 2 else np.array([0.3, -0.25, 0.2]) + rng.uniform(-0.15, 0.15, size=3)
            nb = np.array([[bb[0, 0], 0, 0], [shear[0] * bb[0, 0], bb[1, 1], 0],
                           [shear[1] * bb[0, 0], shear[2] * bb[1, 1], bb[2, 2]]])
            centres = x[0::3]
            move = (centres @ np.linalg.inv(bb)) @ nb - centres
            x = x + np.repeat(move, 3, axis=0)
            bb = nb
        if b == 1:
            for i in range(0, n, 5):
                x[i] += bb[(i // 5) % 3] * (1 if (i // 5) % 2 == 0 else -1)
        confs[b], boxes[b] = x, bb
    return np.ascontiguousarray(confs), np.ascontiguousarray(boxes)


def _min_image(d, box):
    """ReferenceForce::getDeltaRPeriodic on an array of difference vectors (rows of box: a, b, c)."""
    d = d.copy()
    d -= np.floor(d[..., 2:3] / box[2, 2] + 0.5) * box[2]
    d -= np.floor(d[..., 1:2] / box[1, 1] + 0.5) * box[1]
    d -= np.floor(d[..., 0:1] / box[0, 0] + 0.5) * box[0]
    return d


def _assert_clear_of_cutoff(force, conf, box):
    """The condition on the inputs: no non-excluded minimum-image pair within 1e-9 nm of the cutoff
    (such a pair could fall on different sides of it in the oracle and in the kernels)."""
    n = len(conf)
    r = np.linalg.norm(_min_image(conf[None, :, :] - conf[:, None, :], box), axis=2)
    skip = np.eye(n, dtype=bool)
    for k in range(force.getNumExceptions()):
        i, j = force.getExceptionParameters(k)
        skip[i, j] = skip[j, i] = True
    gap = np.abs(r - force.getCutoffDistance())[~skip]
    assert gap.size == 0 or gap.min() > 1e-9, gap.min()


def _cotangents(n, seed, nconf=B):
    """{set: (e_bar, q_bar, f_bar)} -- E only, q only, F only, all three; seeded normal values."""
    rng = np.random.default_rng(seed)
    eb, qb, fb = rng.normal(size=nconf), rng.normal(size=(nconf, n)), rng.normal(size=(nconf, n, 3))
    return {"E": (eb, None, None), "q": (None, qb, None), "F": (None, None, fb), "EqF": (eb, qb, fb)}


def _counts(force):
    return (force.getNumParticles(), 2 * force.getNumFluxBonds(), 2 * force.getNumFluxAngles(),
            5 * force.getNumFluxWaters())


def _perturbed(force, p, delta):
    """A deep copy of force with flat parameter p (the cf_params order) moved by delta."""
    f = copy.deepcopy(force)
    n, b2, a2, w5 = _counts(f)
    if p < n:
        f._charges[p] += delta
        return f
    p -= n
    for store, width, size in ((f._fbond_par, 2, b2), (f._fangle_par, 2, a2), (f._fwater_par, 5, w5)):
        if p < size:
            row = list(store[p // width])
            row[p % width] += delta
            store[p // width] = tuple(row)
            return f
        p -= size
    raise IndexError("parameter index out of range")


def _loss(res, cot, b):
    eb, qb, fb = cot
    v = 0.0
    if eb is not None:
        v += eb[b] * res["energy"]
    if qb is not None:
        v += float(np.dot(qb[b], res["charges"]))
    if fb is not None:
        v += float(np.sum(fb[b] * res["forces"]))
    return v


def _fd(force, box, confs, boxes, cots, params, checked):
    """Central differences of the oracle: {set: (len(checked), len(params))}.  One oracle per
    perturbed force (the default box fixes alpha and kmax), shared by the conformations and the
    cotangent sets."""
    for b in checked:
        _assert_clear_of_cutoff(force, confs[b], boxes[b])
    out = {s: np.zeros((len(checked), len(params))) for s in SETS}
    for col, p in enumerate(params):
        res = []
        for sign in (1.0, -1.0):
            o = Oracle(_perturbed(force, p, sign * H_FD), box)
            res.append([o.execute(confs[b], boxes[b]) for b in checked])
        for s in SETS:
            for row, b in enumerate(checked):
                out[s][row, col] = (_loss(res[0][row], cots[s], b) - _loss(res[1][row], cots[s], b)) / (2 * H_FD)
    return out


def _sample(force, seed):
    """64 parameters, at least 8 of each kind present."""
    rng = np.random.default_rng(seed)
    counts = _counts(force)
    picked, start = [], 0
    for cnt in counts:
        if cnt:
            picked += list(start + rng.choice(cnt, size=min(8, cnt), replace=False))
        start += cnt
    rest = np.setdiff1d(np.arange(sum(counts)), picked)
    picked += list(rng.choice(rest, size=64 - len(picked), replace=False))
    return sorted(int(p) for p in picked)


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """(system, force, default box, conformations, boxes, cotangents)"""
    system, force, pos, box = _system(name)
    confs, boxes = _conformations(name, pos, box, 400 + SYSTEMS.index(name))
    if name == "aniso":
        assert len(set(Oracle(force, box).ewald()[1])) == 3
    if name == "tric":
        assert [b for b in range(B) if not (boxes[b][1, 0] or boxes[b][2, 0] or boxes[b][2, 1])] == [2]
    return system, force, box, confs, boxes, _cotangents(len(pos), 51 + SYSTEMS.index(name))


@functools.lru_cache(maxsize=None)
def _case(name):
    """_inputs + (checked parameters, checked conformations, fd): the finite differences run once
    per system and are shared, read-only."""
    system, force, box, confs, boxes, cots = _inputs(name)
    if name in SAMPLED:
        params, checked = _sample(force, 7 + SYSTEMS.index(name)), [0]
    else:
        params, checked = list(range(sum(_counts(force)))), list(range(B))
    return system, force, box, confs, boxes, cots, params, checked, _fd(force, box, confs, boxes, cots, params, checked)


def _kernel(name, **kw):
    system, force = _inputs(name)[:2]
    return HipCalcCoulForceKernel(**kw).initialize(system, force)


def _check_against_fd(tag, k, confs, boxes, cots, params, checked, fd):
    for s in SETS:
        g = k.execute_batch_vjp_host(confs, *cots[s], boxes=boxes)["flat"]
        assert np.isfinite(g).all()
        err = np.abs(g[checked][:, params] - fd[s]).max()
        scale = np.abs(g[checked]).max()
        ratio = f"{err / scale:.3e}" if scale > 0 else "-"
        print(f"{tag} [{s}]: max|grad - fd| = {err:.3e}, max|grad| = {scale:.3e}, ratio = {ratio}")
        assert err <= REL * scale + ABS, (tag, s, err, scale)
    assert k.device_errors() == 0


# 1 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SYSTEMS)
def test_matches_central_differences_of_the_oracle(name):
    system, force, box, confs, boxes, cots, params, checked, fd = _case(name)
    k = _kernel(name)
    assert k.param_counts() == _counts(force)
    if name in SAMPLED:
        counts = _counts(force)
        edges = np.cumsum((0,) + counts)
        for kind in range(4):
            if counts[kind]:
                assert sum(edges[kind] <= p < edges[kind + 1] for p in params) >= 8
        assert len(params) == 64 and checked == [0]
    _check_against_fd(name, k, confs, boxes, cots, params, checked, fd)
    if name == "w1":   # every pair excluded, and still the energy and the forces depend on the parameters:
        for s in ("E", "F"):   # self term, k-space and the erf correction are functions of q
            g = k.execute_batch_vjp_host(confs, *cots[s], boxes=boxes)["flat"]
            assert np.abs(g).max() > 0.0


# 2 ------------------------------------------------------------------------------------------
def test_terms_with_k_zero():
    system, force, box, confs, boxes, cots = _inputs("w22")
    force = copy.deepcopy(force)
    force._fbond_par[0] = (0.0, force._fbond_par[0][1])
    force._fangle_par[0] = (0.0, force._fangle_par[0][1])
    k1, k2, kub, b0, ub0 = force._fwater_par[0]
    force._fwater_par[0] = (0.0, 0.0, 0.0, b0, ub0)
    params = list(range(sum(_counts(force))))
    k = HipCalcCoulForceKernel().initialize(system, force)
    _check_against_fd("w22, k = 0", k, confs, boxes, cots, params, [1],
                      _fd(force, box, confs, boxes, cots, params, [1]))


# 3 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["w22", "w100"])
def test_linearity_and_null_cotangents(name):
    system, force, box, confs, boxes, cots = _inputs(name)
    k = _kernel(name, kspace_algo=HipCalcCoulForceKernel.KSPACE_EXACT_MFMA)
    g = {s: k.execute_batch_vjp_host(confs, *cots[s], boxes=boxes)["flat"] for s in SETS}
    total = g["E"] + g["q"] + g["F"]
    d = np.abs(g["EqF"] - total).max()
    print(f"{name}: linearity max|d| = {d:.3e}, max|grad| = {np.abs(g['EqF']).max():.3e}")
    assert d <= 1e-12 * np.abs(g["EqF"]).max()
    # no cotangent: exact zeros, whatever the array held
    stats = k.batch_stats()
    out = k.execute_batch_vjp_host(confs, boxes=boxes)
    assert np.array_equal(out["flat"], np.zeros((B, sum(_counts(force)))))
    n = confs.shape[1]
    pt = torch.tensor(confs, device="cuda:0")
    gt = torch.full((B, sum(_counts(force))), 7.0, dtype=torch.float64, device="cuda:0")
    k.execute_batch_vjp_device(pt, gt, boxes=boxes)
    k.synchronize()
    assert (gt == 0.0).all()
    assert k.batch_stats() == (stats[0] + 2, stats[1] + 2 * B, stats[2])   # calls and conformations, no pass
    # the views
    assert out["charges"].shape == (B, n) and out["bonds"].shape == (B, force.getNumFluxBonds(), 2)
    assert out["angles"].shape == (B, force.getNumFluxAngles(), 2)
    assert out["waters"].shape == (B, force.getNumFluxWaters(), 5)
    assert all(np.shares_memory(out[key], out["flat"]) for key in ("charges", "bonds", "angles", "waters"))
    # e_bar = 1 alone: the charges block is dE/dq of cf_compute with that box and the exact k-sum
    ge = k.execute_batch_vjp_host(confs, energy_bar=np.ones(B), boxes=boxes)
    for b in range(B):
        k.execute_host(confs[b], boxes[b])
        dedq = k.dedq()
        dd = np.abs(ge["charges"][b] - dedq).max()
        print(f"{name} conformation {b}: max|a - dedq| = {dd:.3e}, max|dedq| = {np.abs(dedq).max():.3e}")
        assert dd <= 1e-12 * np.abs(dedq).max() + 1e-10
    assert k.device_errors() == 0


# 4 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ions", "w100", "tric"])
def test_bitwise_guarantees(name):
    stream = torch.cuda.Stream()
    system, force, box, confs, boxes, cots = _inputs(name)
    k = _kernel(name, stream=stream.cuda_stream)
    for s in ("E", "EqF"):
        cot = cots[s]
        c0, n0, p0 = k.batch_stats()
        g = k.execute_batch_vjp_host(confs, *cot, boxes=boxes)["flat"]
        assert k.batch_stats() == (c0 + 1, n0 + B, p0 + 1)      # one pass under the automatic limit
        assert np.array_equal(k.execute_batch_vjp_host(confs, *cot, boxes=boxes)["flat"], g)
        for b in range(B):                                      # alone (B = 1) = its row of the batch
            one = [None if t is None else np.ascontiguousarray(t[b:b + 1]) for t in cot]
            gb = k.execute_batch_vjp_host(np.ascontiguousarray(confs[b:b + 1]), *one, boxes=boxes[b])["flat"]
            assert np.array_equal(gb[0], g[b])
        rev = [None if t is None else np.ascontiguousarray(t[::-1]) for t in cot]
        gr = k.execute_batch_vjp_host(np.ascontiguousarray(confs[::-1]), *rev,
                                      boxes=np.ascontiguousarray(boxes[::-1]))["flat"]
        assert np.array_equal(gr[::-1], g)
        p1 = k.batch_stats()[2]
        k.set_batch_limit(2)
        g2 = k.execute_batch_vjp_host(confs, *cot, boxes=boxes)["flat"]
        assert k.batch_stats()[2] == p1 + 2                     # 2 + 1 conformations
        assert np.array_equal(g2, g)
        k.set_batch_limit(0)
        # the device form on the side stream
        dev = lambda a: None if a is None else torch.tensor(a, device="cuda:0")
        pt, ct = dev(confs), [dev(t) for t in cot]
        gt = torch.full(g.shape, -3.0, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()   # the inputs exist before the side stream reads them
        bx = boxes.copy()
        k.execute_batch_vjp_device(pt, gt, *ct, boxes=bx)
        bx[:] = np.nan             # the boxes are the caller's again as soon as the call returns
        stream.synchronize()
        assert np.array_equal(gt.cpu().numpy(), g)
    assert k.device_errors() == 0


# 5 ------------------------------------------------------------------------------------------
def test_isolation_from_the_single_evaluation_state_and_the_forward_batch():
    system, force, box, confs, boxes, cots = _inputs("w100")
    k = _kernel("w100", kspace_algo=HipCalcCoulForceKernel.KSPACE_GRID)
    k.set_graph(True)
    e0, f0 = k.execute_host(confs[0], boxes[0])
    e0, f0 = k.execute_host(confs[0], boxes[0])
    e, f, q = k.execute_batch_host(confs, boxes=boxes)
    diag = (k.charges(), k.dedq(), k.energy_terms(), k.neighbor_stats(), k.graph_stats())
    stats = k.batch_stats()
    g = k.execute_batch_vjp_host(confs, *cots["EqF"], boxes=boxes)["flat"]
    assert k.batch_stats() == (stats[0] + 1, stats[1] + B, stats[2] + 1)
    after = (k.charges(), k.dedq(), k.energy_terms(), k.neighbor_stats(), k.graph_stats())
    for a, b in zip(diag[:3], after[:3]):
        assert np.array_equal(a, b)
    assert diag[3:] == after[3:]
    e1, f1 = k.execute_host(confs[0], boxes[0])
    assert e1 == e0 and np.array_equal(f1, f0)
    # the forward periodic batch and the gradients share a workspace: neither disturbs the other
    e2, f2, q2 = k.execute_batch_host(confs, boxes=boxes)
    assert np.array_equal(e, e2) and np.array_equal(f, f2) and np.array_equal(q, q2)
    assert np.array_equal(k.execute_batch_vjp_host(confs, *cots["EqF"], boxes=boxes)["flat"], g)
    assert k.device_errors() == 0


# 6 ------------------------------------------------------------------------------------------
def test_parameter_update_reaches_the_gradient_path():
    system, force, pos, box = _system("w22", seed=5)
    force = copy.deepcopy(force)
    confs, boxes = _conformations("w22", pos, box, 11)
    cots = _cotangents(pos.shape[0], 13)
    k = HipCalcCoulForceKernel().initialize(system, force)
    g0 = k.execute_batch_vjp_host(confs, *cots["EqF"], boxes=boxes)["flat"]
    for i in range(force.getNumParticles()):
        q, s, e = force.getParticleParameters(i)
        force.setParticleParameters(i, q * 1.05, s, e)
    for w in range(force.getNumFluxWaters()):
        k1, k2, kub, b0, ub0 = force._fwater_par[w]
        force._fwater_par[w] = (k1 * 1.1, k2, kub, b0, ub0)
    k.copyParametersToContext(force)
    g1 = k.execute_batch_vjp_host(confs, *cots["EqF"], boxes=boxes)["flat"]
    assert np.abs(g1 - g0).max() > 1e-3 * np.abs(g0).max()   # the update took effect
    params = list(range(sum(_counts(force))))
    _check_against_fd("w22, updated", k, confs, boxes, cots, params, [1],
                      _fd(force, box, confs, boxes, cots, params, [1]))


# 7 ------------------------------------------------------------------------------------------
def test_argument_errors():
    lib = _cabi.load_library()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    # a non-periodic handle with boxes
    system, force, cpos, _ = ts.cluster_c1()
    kn = HipCalcCoulForceKernel().initialize(system, force)
    with pytest.raises(ChargeFluxError) as ei:
        kn.execute_batch_vjp_host(np.ascontiguousarray(cpos[None]), energy_bar=np.ones(1),
                                  boxes=np.diag([3.0, 3.0, 3.0]))
    assert ei.value.code == _cabi.CF_ERR_INVALID and "periodic" in str(ei.value)
    assert kn.device_errors() == 0
    # a bad box (cutoff above half a diagonal) in conformation 1: names it, touches nothing, counts nothing
    system, force, box, confs, boxes, cots = _inputs("w22")
    k = _kernel("w22")
    n, np_ = confs.shape[1], sum(_counts(force))
    g = k.execute_batch_vjp_host(confs, *cots["EqF"], boxes=boxes)["flat"]
    stats = k.batch_stats()
    bad = boxes.copy()
    bad[1] = np.diag([0.9, 0.77, 0.9])                     # cutoff 0.39 > 0.385
    pt = torch.tensor(confs, device="cuda:0")
    eb = torch.ones(B, dtype=torch.float64, device="cuda:0")
    gt = torch.full((B, np_), 2.0, dtype=torch.float64, device="cuda:0")

    def untouched():
        k.synchronize()
        return bool((gt == 2.0).all()) and k.batch_stats() == stats

    with pytest.raises(ChargeFluxError) as ei:
        k.execute_batch_vjp_device(pt, gt, eb, boxes=bad)
    assert ei.value.code == _cabi.CF_ERR_INVALID and "conformation 1" in str(ei.value)
    assert untouched()
    with pytest.raises(ChargeFluxError) as ei:
        k.execute_batch_vjp_host(confs, energy_bar=np.ones(B), boxes=bad)
    assert ei.value.code == _cabi.CF_ERR_INVALID and "conformation 1" in str(ei.value)
    assert untouched()
    # NULL positions, boxes or grad and a negative nconf at the C level; nconf = 0
    bp = boxes.ctypes.data_as(C.POINTER(C.c_double))
    cp = confs.ctypes.data_as(C.POINTER(C.c_double))
    vjp, vjp_host = lib.cf_compute_batch_periodic_vjp, lib.cf_compute_batch_periodic_vjp_host
    assert vjp(k._h, B, None, bp, ptr(eb), None, None, ptr(gt)) == _cabi.CF_ERR_INVALID
    assert vjp(k._h, B, ptr(pt), None, ptr(eb), None, None, ptr(gt)) == _cabi.CF_ERR_INVALID
    assert vjp(k._h, B, ptr(pt), bp, ptr(eb), None, None, None) == _cabi.CF_ERR_INVALID
    assert vjp(k._h, -1, ptr(pt), bp, ptr(eb), None, None, ptr(gt)) == _cabi.CF_ERR_INVALID
    gh = np.full((B, np_), 2.0)
    ghp = gh.ctypes.data_as(C.POINTER(C.c_double))
    assert vjp_host(k._h, B, None, bp, None, None, None, ghp) == _cabi.CF_ERR_INVALID
    assert vjp_host(k._h, B, cp, None, None, None, None, ghp) == _cabi.CF_ERR_INVALID
    assert vjp_host(k._h, B, cp, bp, None, None, None, None) == _cabi.CF_ERR_INVALID
    assert vjp_host(k._h, -1, cp, bp, None, None, None, ghp) == _cabi.CF_ERR_INVALID
    assert vjp(k._h, 0, ptr(pt), bp, ptr(eb), None, None, ptr(gt)) == _cabi.CF_OK
    assert vjp_host(k._h, 0, cp, bp, None, None, None, ghp) == _cabi.CF_OK
    assert untouched() and (gh == 2.0).all()
    assert k.execute_batch_vjp_host(np.zeros((0, n, 3)), boxes=np.zeros((0, 3, 3)))["flat"].shape == (0, np_)
    assert k.batch_stats() == stats
    # between cf_compute_begin and _end
    k.begin(pt[0], boxes[0])
    with pytest.raises(ChargeFluxError) as ei:
        k.execute_batch_vjp_device(pt, gt, eb, boxes=boxes)
    assert ei.value.code == _cabi.CF_ERR_STATE
    k.end()
    assert untouched()
    # the call still works after all that, with the same bits
    assert np.array_equal(k.execute_batch_vjp_host(confs, *cots["EqF"], boxes=boxes)["flat"], g)
    assert k.device_errors() == 0
    # several ranks
    system, force, box, confs2, boxes2, _ = _inputs("w100")
    k2 = HipCalcCoulForceKernel(rank=0, world_size=2).initialize(system, force)
    with pytest.raises(ChargeFluxError) as ei:
        k2.execute_batch_vjp_host(confs2, energy_bar=np.ones(B), boxes=boxes2)
    assert ei.value.code == _cabi.CF_ERR_STATE


# 8 ------------------------------------------------------------------------------------------
def _model(system, force, pos, box, name, nconf, seed):
    from openmmcoul.fitting import BatchedChargeFlux
    force = copy.deepcopy(force)
    k = HipCalcCoulForceKernel().initialize(system, force)
    confs, boxes = _conformations(name, pos, box, seed, nconf)
    return BatchedChargeFlux(k, force), torch.tensor(confs, device="cuda:0"), boxes


def test_autograd_gradcheck():
    # 2 waters (one FluxWater, one bond + angle) in a 0.39 nm box, cutoff below half of every scaled box
    model, pos, boxes = _model(*ts.water_box(2, cutoff=0.17, every_bond_angle=2), "w2", 2, 3)
    assert not np.array_equal(boxes[0], boxes[1])
    params = model.parameters(device="cuda:0")
    assert [tuple(p.shape) for p in params] == [(6,), (2, 2), (1, 2), (1, 5)]
    keep = boxes.copy()
    fn = lambda q, b, a, w: model(q, b, a, w, pos, boxes=boxes)
    assert torch.autograd.gradcheck(fn, params, eps=1e-3, atol=1e-7, rtol=1e-7)
    assert np.array_equal(boxes, keep)
    # backward uses the boxes of its forward, whatever became of the caller's array
    out = model(*params, pos, boxes=boxes)[1].square().sum()
    boxes[:] = np.nan
    grads = torch.autograd.grad(out, params)
    assert all(torch.isfinite(t).all() for t in grads)
    with pytest.raises(ValueError):
        model(*params, pos.clone().requires_grad_(True), boxes=keep)


def test_adam_lowers_a_force_matching_loss():
    model, pos, boxes = _model(*_system("w22"), "w22", 4, 9)
    start = [p.detach().clone() for p in model.parameters(device="cuda:0")]
    rng = np.random.default_rng(1)
    with torch.no_grad():
        truth = [p * torch.tensor(1 + 0.05 * rng.uniform(-1, 1, size=tuple(p.shape)), device=p.device) for p in start]
        target = model(*truth, pos, boxes=boxes)[1]
    params = [p.clone().requires_grad_(True) for p in start]
    opt = torch.optim.Adam(params, lr=2e-4)
    losses = []
    for _ in range(4):
        opt.zero_grad()
        loss = ((model(*params, pos, boxes=boxes)[1] - target) ** 2).mean()
        losses.append(loss.item())
        loss.backward()
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in params)
        opt.step()
    print("force-matching loss:", " ".join(f"{v:.6e}" for v in losses))
    assert losses[1] < losses[0] and losses[2] < losses[1] and losses[3] < losses[2]
