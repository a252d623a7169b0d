"""GPU tests of the periodic batched evaluation (cf_compute_batch_periodic, include/chargeflux.h;
DESIGN.md §4.6 "Batched, periodic"): B conformations of a periodic system, each with its own box, in
one call -- against the oracle and against cf_compute (exact k-sum) one conformation at a time, plus
the bitwise guarantees (independence of the batch, of B, of the pass size, host = device form),
isolation from the single-evaluation state on differently configured handles, parameter updates
and the argument errors.

Conformations: base positions + N(0, 0.003 nm) jitter; each has its own box, the default box
scaled per axis by factors in [0.95, 1.05] with the positions scaled along; in the odd ones every
fifth atom is moved by a whole box vector (molecules split across images).  Every cutoff is <= 0.45
of the smallest default box length, so the shrunken boxes still pass the half-box rule.

Tolerances are the fp64 bars of test_gpu_parity.py / test_gpu_batch.py:
  forces   max |dF| <= 1e-8 kJ/mol/nm,  energy |dE| <= 1e-9 |E| + 1e-8 kJ/mol,  charges <= 1e-12 e
"""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import Oracle  # noqa: E402
from openmmcoul import ChargeFluxError, CoulForce, HipCalcCoulForceKernel, System, _cabi  # noqa: E402
from openmmcoul import testsystems as ts  # noqa: E402

F_TOL = 1e-8
Q_TOL = 1e-12
B = 7
FLAGS = [(True, True), (True, False), (False, True)]
SYSTEMS = ["w1", "ions", "w22", "w100", "aniso", "tric"]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _e_tol(e):
    return 1e-9 * abs(e) + 1e-8


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


def _system(name):
    if name == "w1":      # fewer atoms than a wave, every pair excluded: self, k-space, exclusions only
        return ts.water_box(1, cutoff=0.13)
    if name == "ions":
        return _ions()
    if name == "w22":     # across one wave; FluxWater mixed with bond and angle terms
        return ts.water_box(22, cutoff=0.39, every_bond_angle=2)
    if name == "w100":    # across a 256-entry j tile with a tail
        return ts.water_box(100, cutoff=0.64)
    if name == "aniso":
        return _aniso()
    if name == "tric":
        return ts.triclinic_water_box(27, cutoff=0.41)
    raise KeyError(name)


def _conformations(name, pos, box, seed):
    """(confs (B,N,3), boxes (B,3,3)).  Box b = the default box with column a scaled by s[b,a] in
    [0.95, 1.05] (per-axis scaling of a reduced box, positions scaled along).  The triclinic system
    also gets its own shears per conformation, within the reduced form, and conformations 2 and 5
    are orthorhombic (molecules moved rigidly with their oxygen's fractional coordinates, so the
    lattice of centres follows the box)."""
    rng = np.random.default_rng(seed)
    n = len(pos)
    confs = np.empty((B, n, 3))
    boxes = np.empty((B, 3, 3))
    for b in range(B):
        s = rng.uniform(0.95, 1.05, size=3)
        x = pos + rng.normal(0.0, 0.003, size=pos.shape)
        bb = box * s[None, :]
        x = x * s[None, :]
        if name == "tric":
            shear = np.zeros(3) if b in (2, 5) else np.array([0.3, -0.25, 0.2]) + rng.uniform(-0.15, 0.15, size=3)
            nb = np.array([[bb[0, 0], 0, 0], [shear[0] * bb[0, 0], bb[1, 1], 0],
                           [shear[1] * bb[0, 0], shear[2] * bb[1, 1], bb[2, 2]]])
            centres = x[0::3]
            move = (centres @ np.linalg.inv(bb)) @ nb - centres
            x = x + np.repeat(move, 3, axis=0)
            bb = nb
        if b % 2 == 1:        # every fifth atom by a whole box vector
            for i in range(0, n, 5):
                x[i] += bb[(i // 5) % 3] * (1 if (i // 5) % 2 == 0 else -1)
        confs[b], boxes[b] = x, bb
    return np.ascontiguousarray(confs), np.ascontiguousarray(boxes)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(system, force, default box, confs, boxes, {(fl, en): [oracle result per conformation]}): the
    oracle runs once per system and is shared, read-only, by every test."""
    system, force, pos, box = _system(name)
    confs, boxes = _conformations(name, pos, box, 300 + SYSTEMS.index(name))
    o = Oracle(force, box)
    if name == "aniso":
        kmax = o.ewald()[1]
        assert len(set(kmax)) == 3, kmax
    if name == "tric":
        ortho = [b for b in range(B) if not (boxes[b][1, 0] or boxes[b][2, 0] or boxes[b][2, 1])]
        assert ortho == [2, 5]
    refs = {fe: [o.execute(confs[b], boxes[b], *fe) for b in range(B)] for fe in FLAGS}
    for r in refs[(True, True)]:
        assert np.isfinite(r["forces"]).all() and np.isfinite(r["energy"])
    return system, force, box, confs, boxes, refs


def _kernel(name, **kw):
    system, force, box, confs, boxes, refs = _case(name)
    return HipCalcCoulForceKernel(**kw).initialize(system, force), confs, boxes, refs


def _report(tag, df, de, dq):
    print(f"{tag}: max|dF| = {df:.3e} kJ/mol/nm, max|dE| = {de:.3e} kJ/mol, max|dq| = {dq:.3e} e")


# 1 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SYSTEMS)
def test_batch_matches_oracle_per_conformation(name):
    k, confs, boxes, refs = _kernel(name)
    n = confs.shape[1]
    for fl, en in FLAGS:
        pre = np.full((B, n, 3), 0.5)
        e, f, q = k.execute_batch_host(confs, fl, en, forces=pre.copy(), boxes=boxes)
        ref = refs[(fl, en)]   # without includeEnergy: the oracle's energy with the reference's quirk
        df = max(np.abs(f[b] - 0.5 - ref[b]["forces"]).max() for b in range(B)) if fl else 0.0
        de = max(abs(e[b] - ref[b]["energy"]) for b in range(B))
        dq = max(np.abs(q[b] - ref[b]["charges"]).max() for b in range(B))
        _report(f"{name} F={fl} E={en}", df, de, dq)
        for b in range(B):
            if fl:
                assert np.abs(f[b] - 0.5 - ref[b]["forces"]).max() <= F_TOL, b
            assert abs(e[b] - ref[b]["energy"]) <= _e_tol(ref[b]["energy"]), (b, e[b], ref[b]["energy"])
            assert np.abs(q[b] - ref[b]["charges"]).max() <= Q_TOL
        if not fl:
            assert np.array_equal(f, pre)     # untouched, bit for bit
    assert k.device_errors() == 0


# 2 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SYSTEMS)
def test_batch_matches_cf_compute_one_at_a_time(name):
    k, confs, boxes, _ = _kernel(name, kspace_algo=HipCalcCoulForceKernel.KSPACE_EXACT_MFMA)
    e, f, q = k.execute_batch_host(confs, boxes=boxes)
    df = de = 0.0
    for b in range(B):
        e1, f1 = k.execute_host(confs[b], boxes[b])
        q1 = k.charges()
        df, de = max(df, np.abs(f[b] - f1).max()), max(de, abs(e[b] - e1))
        assert np.abs(f[b] - f1).max() <= F_TOL, b
        assert abs(e[b] - e1) <= _e_tol(e1), b
        assert np.array_equal(q[b], q1), b
    _report(f"{name} vs cf_compute", df, de, 0.0)
    assert k.device_errors() == 0


# 3 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["w22", "tric"])
def test_independence_and_determinism_bitwise(name):
    stream = torch.cuda.Stream()
    k, confs, boxes, _ = _kernel(name, stream=stream.cuda_stream)
    n = confs.shape[1]
    c0, n0, p0 = k.batch_stats()
    e, f, q = k.execute_batch_host(confs, boxes=boxes)
    assert k.batch_stats() == (c0 + 1, n0 + B, p0 + 1)     # one pass under the automatic limit
    for b in range(B):                                     # alone (B = 1) = its slice of the batch
        eb, fb, qb = k.execute_batch_host(np.ascontiguousarray(confs[b:b + 1]), boxes=boxes[b])
        assert np.array_equal(eb[0], e[b]) and np.array_equal(fb[0], f[b]) and np.array_equal(qb[0], q[b])
    assert k.batch_stats() == (c0 + 1 + B, n0 + 2 * B, p0 + 1 + B)
    # a different batch around it: reversed order
    er, fr, qr = k.execute_batch_host(np.ascontiguousarray(confs[::-1]), boxes=np.ascontiguousarray(boxes[::-1]))
    assert np.array_equal(er[::-1], e) and np.array_equal(fr[::-1], f) and np.array_equal(qr[::-1], q)
    for lim, passes in ((1, B), (3, 3)):                   # 7 x 1; 3 + 3 + 1 conformations
        p1 = k.batch_stats()[2]
        k.set_batch_limit(lim)
        e3, f3, q3 = k.execute_batch_host(confs, boxes=boxes)
        assert k.batch_stats()[2] == p1 + passes
        assert np.array_equal(e, e3) and np.array_equal(f, f3) and np.array_equal(q, q3)
    k.set_batch_limit(0)
    # the device form on the side stream
    pt = torch.tensor(confs, device="cuda:0")
    ft = torch.zeros((B, n, 3), dtype=torch.float64, device="cuda:0")
    et = torch.zeros(B, dtype=torch.float64, device="cuda:0")
    qt = torch.zeros((B, n), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()   # the inputs exist before the side stream reads them
    bx = boxes.copy()
    k.execute_batch_device(pt, True, True, ft, et, qt, boxes=bx)
    bx[:] = np.nan             # the boxes are the caller's again as soon as the call returns
    stream.synchronize()
    assert np.array_equal(et.cpu().numpy(), e)
    assert np.array_equal(ft.cpu().numpy(), f)
    assert np.array_equal(qt.cpu().numpy(), q)
    assert k.device_errors() == 0


# 4 ------------------------------------------------------------------------------------------
def test_isolation_from_the_single_evaluation_state():
    system, force, box, confs, boxes, refs = _case("w100")
    base = None
    for kw, skin in ((dict(), 0.0), (dict(kspace_algo=HipCalcCoulForceKernel.KSPACE_GRID), 0.0),
                     (dict(precision="mixed"), 0.0), (dict(), 0.02)):
        k = HipCalcCoulForceKernel(**kw).initialize(system, force)
        if skin:
            k.set_neighbor_skin(skin)
        e0, f0 = k.execute_host(confs[0], boxes[0])
        diag = (k.charges(), k.dedq(), k.energy_terms(), k.neighbor_stats(), k.graph_stats())
        e, f, q = k.execute_batch_host(confs[1:], boxes=np.ascontiguousarray(boxes[1:]))
        after = (k.charges(), k.dedq(), k.energy_terms(), k.neighbor_stats(), k.graph_stats())
        for a, b in zip(diag[:3], after[:3]):
            assert np.array_equal(a, b)
        assert diag[3:] == after[3:]
        e1, f1 = k.execute_host(confs[0], boxes[0])
        assert e1 == e0 and np.array_equal(f1, f0)
        # the batch result does not depend on how the handle was configured
        if base is None:
            base = (e, f, q)
            ref = refs[(True, True)]
            for b in range(1, B):
                assert np.abs(f[b - 1] - ref[b]["forces"]).max() <= F_TOL
                assert abs(e[b - 1] - ref[b]["energy"]) <= _e_tol(ref[b]["energy"])
        else:
            assert np.array_equal(e, base[0]) and np.array_equal(f, base[1]) and np.array_equal(q, base[2])
        assert k.device_errors() == 0
        k.destroy()


# 5 ------------------------------------------------------------------------------------------
def test_parameter_update_reaches_the_batch_path():
    system, force, pos, box = ts.water_box(22, cutoff=0.39, every_bond_angle=2, seed=5)
    confs, boxes = _conformations("w22", pos, box, 11)
    k = HipCalcCoulForceKernel().initialize(system, force)
    e0, f0, q0 = k.execute_batch_host(confs, boxes=boxes)
    for w in range(force.getNumFluxWaters()):
        k1, k2, kub, b0, ub0 = force._fwater_par[w]
        force._fwater_par[w] = (k1 * 1.1, k2 * 0.9, kub, b0, ub0)
    k.copyParametersToContext(force)
    e, f, q = k.execute_batch_host(confs, boxes=boxes)
    assert np.abs(q - q0).max() > 1e-6                      # the update took effect
    o = Oracle(force, box)
    for b in range(B):
        ref = o.execute(confs[b], boxes[b])
        assert np.abs(f[b] - ref["forces"]).max() <= F_TOL
        assert abs(e[b] - ref["energy"]) <= _e_tol(ref["energy"])
        assert np.abs(q[b] - ref["charges"]).max() <= Q_TOL
    assert k.device_errors() == 0


# 6 ------------------------------------------------------------------------------------------
def test_argument_errors():
    lib = _cabi.load_library()
    k, confs, boxes, _ = _kernel("w22")
    n = confs.shape[1]
    e, f, q = k.execute_batch_host(confs, boxes=boxes)
    stats = k.batch_stats()
    # one box below twice the cutoff: names its index, touches no output, counts nothing
    bad = boxes.copy()
    bad[4] = np.diag([0.9, 0.77, 0.9])                     # cutoff 0.39 > 0.385
    pre = np.full((B, n, 3), 0.25)
    pt = torch.tensor(confs, device="cuda:0")
    ft = torch.full((B, n, 3), 2.0, dtype=torch.float64, device="cuda:0")
    et = torch.full((B,), 3.0, dtype=torch.float64, device="cuda:0")
    qt = torch.full((B, n), 4.0, dtype=torch.float64, device="cuda:0")

    def untouched():
        k.synchronize()
        return bool((ft == 2.0).all() and (et == 3.0).all() and (qt == 4.0).all()) and k.batch_stats() == stats

    with pytest.raises(ChargeFluxError) as ei:
        k.execute_batch_device(pt, True, True, ft, et, qt, boxes=bad)
    assert ei.value.code == _cabi.CF_ERR_INVALID and "conformation 4" in str(ei.value)
    assert untouched()
    fh = pre.copy()
    with pytest.raises(ChargeFluxError) as ei:
        k.execute_batch_host(confs, forces=fh, boxes=bad)
    assert ei.value.code == _cabi.CF_ERR_INVALID and "conformation 4" in str(ei.value)
    assert np.array_equal(fh, pre) and k.batch_stats() == stats
    # a box that is not in reduced form
    bad = boxes.copy()
    bad[6][0, 1] = 0.1
    with pytest.raises(ChargeFluxError) as ei:
        k.execute_batch_device(pt, True, True, ft, et, qt, boxes=bad)
    assert ei.value.code == _cabi.CF_ERR_INVALID and "conformation 6" in str(ei.value) and "reduced" in str(ei.value)
    bad = boxes.copy()
    bad[0][1, 0] = 0.6 * bad[0][0, 0]                      # |bx| > ax / 2
    with pytest.raises(ChargeFluxError) as ei:
        k.execute_batch_device(pt, True, True, ft, et, qt, boxes=bad)
    assert ei.value.code == _cabi.CF_ERR_INVALID and "conformation 0" in str(ei.value)
    assert untouched()
    # NULL boxes, NULL positions, negative nconf at the C level; nconf = 0
    ptr = lambda t: C.c_void_p(t.data_ptr())
    bp = boxes.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.cf_compute_batch_periodic(k._h, B, ptr(pt), None, 3, ptr(ft), ptr(et), ptr(qt)) == _cabi.CF_ERR_INVALID
    assert lib.cf_compute_batch_periodic(k._h, B, None, bp, 3, ptr(ft), ptr(et), ptr(qt)) == _cabi.CF_ERR_INVALID
    assert lib.cf_compute_batch_periodic(k._h, -1, ptr(pt), bp, 3, ptr(ft), ptr(et), ptr(qt)) == _cabi.CF_ERR_INVALID
    assert lib.cf_compute_batch_periodic_host(k._h, B, None, bp, 3, None, None, None) == _cabi.CF_ERR_INVALID
    assert lib.cf_compute_batch_periodic_host(k._h, B, confs.ctypes.data_as(C.POINTER(C.c_double)), None, 3, None,
                                              None, None) == _cabi.CF_ERR_INVALID
    assert lib.cf_compute_batch_periodic(k._h, 0, ptr(pt), bp, 3, ptr(ft), ptr(et), ptr(qt)) == _cabi.CF_OK
    assert untouched()
    e0, f0, q0 = k.execute_batch_host(np.zeros((0, n, 3)), boxes=np.zeros((0, 3, 3)))
    assert e0.shape == (0,) and f0.shape == (0, n, 3) and q0.shape == (0, n)
    assert k.batch_stats() == stats
    # between cf_compute_begin and _end
    k.begin(pt[0], boxes[0])
    with pytest.raises(ChargeFluxError) as ei:
        k.execute_batch_device(pt, True, True, ft, et, qt, boxes=boxes)
    assert ei.value.code == _cabi.CF_ERR_STATE
    k.end()
    assert untouched()
    # the call still works after all that, with the same bits
    e2, f2, q2 = k.execute_batch_host(confs, boxes=boxes)
    assert np.array_equal(e2, e) and np.array_equal(f2, f) and np.array_equal(q2, q)
    assert k.device_errors() == 0
    # a non-periodic handle with boxes; the non-periodic entry point on a periodic handle is as it was
    system, force, cpos, _ = ts.cluster_c1()
    kn = HipCalcCoulForceKernel().initialize(system, force)
    with pytest.raises(ChargeFluxError) as ei:
        kn.execute_batch_host(np.ascontiguousarray(cpos[None]), boxes=np.diag([3.0, 3.0, 3.0]))
    assert ei.value.code == _cabi.CF_ERR_INVALID and "periodic" in str(ei.value)
    assert kn.device_errors() == 0
    # several ranks
    system, force, box, confs2, boxes2, _ = _case("w100")
    k2 = HipCalcCoulForceKernel(rank=0, world_size=2).initialize(system, force)
    with pytest.raises(ChargeFluxError) as ei:
        k2.execute_batch_host(confs2, boxes=boxes2)
    assert ei.value.code == _cabi.CF_ERR_STATE
