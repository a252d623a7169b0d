"""GPU tests of the LJ sigma / epsilon gradients of the batches (cf_compute_batch_lj_vjp,
include/chargeflux.h; DESIGN.md "Batched, LJ parameter gradients"): against the numpy closed form and
against Richardson-extrapolated central differences of the oracle (tests/lj_reference.py), the
eps = 0 convention, linearity in the cotangents and the NULL case, the bitwise guarantees, parameter
updates, isolation from the single-evaluation state, the argument errors and the torch autograd layer
(openmmcoul.fitting with sigmas= and epsilons=).

Systems: non-periodic clusters by the `_cluster` recipe of the batch tests (waters, ions) -- (1, 0)
every pair excluded, (0, 5) no exclusions and N < 64, (2, 1), (21, 7) across two 64-atom blocks,
(100, 21) a 256-entry j tile with a tail, and a (21, 7) variant with one ion at sigma = 0, eps > 0 and
one at eps = 0, sigma > 0.  Periodic: water_box(8, cutoff 0.3); water_box(27, cutoff 0.4) with a box per
conformation scaled per axis by factors in [0.95, 1.05] (positions scaled along); the triclinic box
of 27 waters at cutoff 0.45; the same system in a batch that mixes triclinic and orthorhombic boxes;
water_box(100, cutoff 0.6).  B = 3 conformations: base + N(0, 0.003 nm) per coordinate, the odd ones
also translated.  Cotangent sets: E only, F only, both.

Bar (both references):  max |grad - ref| <= 1e-9 max |grad| + 1e-9, the maxima per system and
cotangent set over the checked conformations.  Every system but (1, 0) must have max |grad| > 1 in
the reference, so that nothing passes on zeros.  The periodic inputs must keep every non-excluded
pair 1e-9 nm clear of the cutoff (a condition on the inputs, asserted: the pair set is then the same
for the oracle, the numpy form and the kernel).  Observed on MI355X (printed by the tests): see
DESIGN.md.
"""
import copy
import ctypes as C
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from openmmcoul import ChargeFluxError, CoulForce, HipCalcCoulForceKernel, System, _cabi  # noqa: E402
from openmmcoul import testsystems as ts  # noqa: E402
from tests import lj_reference as ljr  # noqa: E402

B = 3
REL, ABS = 1e-9, 1e-9
SHIFT = np.array([0.4, -0.2, 0.1])
SETS = ("E", "F", "EF")
CLUSTERS = ["c1+0", "c0+5", "c2+1", "c21+7", "c100+21", "c21+7v"]
BOXES = ["w8", "w27s", "tric27", "mix", "w100"]
SYSTEMS = CLUSTERS + BOXES
SAMPLED = ("c100+21", "w100")   # 32 sampled parameters of conformation 0


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _cluster(nw, ni, seed=ts.SEED):
    rng = np.random.default_rng(seed + 1000 * nw + ni)
    a = 0.325
    m = max(1, int(math.ceil(max(nw, ni) ** (1.0 / 3.0) - 1e-9)))
    grid = np.array([(i, j, k) for i in range(m) for j in range(m) for k in range(m)], dtype=np.float64)
    wcent = (grid[:nw] + 0.25) * a + rng.uniform(-0.02, 0.02, size=(nw, 3))
    icent = (grid[:ni] + 0.75) * a + rng.uniform(-0.02, 0.02, size=(ni, 3))
    wpos = ts._water_geometry(rng, wcent).reshape(-1, 3)
    force, system = CoulForce(), System()
    for w in range(nw):
        for q, s, e, mass in ((ts.Q_O, ts.SIG_O, ts.EPS_O, 15.999), (ts.Q_H, 0.0, 0.0, 1.008), (ts.Q_H, 0.0, 0.0, 1.008)):
            force.addParticle(q, s, e)
            system.addParticle(mass)
    for w in range(nw):
        ts.add_water(force, 3 * w, w % 2 == 1)
    for i in range(ni):
        force.addParticle(1.0 if i % 2 == 0 else -1.0, 0.3, 0.5)
        system.addParticle(22.99 if i % 2 == 0 else 35.45)
    system.addForce(force)
    return system, force, np.concatenate([wpos, icent])


def _system(name):
    """(system, force, positions, default box or None)"""
    if name in CLUSTERS:
        nw, ni = (int(v) for v in name[1:].rstrip("v").split("+"))
        system, force, pos = _cluster(nw, ni)
        if name.endswith("v"):   # ion 0: sigma = 0, eps > 0; ion 1: eps = 0, sigma > 0
            q, s, e = force.getParticleParameters(3 * nw)
            force.setParticleParameters(3 * nw, q, 0.0, e)
            q, s, e = force.getParticleParameters(3 * nw + 1)
            force.setParticleParameters(3 * nw + 1, q, s, 0.0)
        return system, force, pos, None
    if name == "w8":
        return ts.water_box(8, cutoff=0.3)
    if name == "w27s":
        return ts.water_box(27, cutoff=0.4)
    if name in ("tric27", "mix"):
        return ts.triclinic_water_box(27, cutoff=0.45)
    if name == "w100":      # across a 256-entry j tile with a tail
        return ts.water_box(100, cutoff=0.6)
    raise KeyError(name)


def _conformations(name, pos, box, seed, nconf=B):
    """(confs (nconf,N,3), boxes (nconf,3,3) or None): base + N(0, 0.003 nm) per coordinate, the odd
    conformations also translated.  w27s: box b is the default box with axis a scaled by s[b,a] in
    [0.95, 1.05], positions scaled along.  mix: conformation 1 in the orthorhombic box of the same
    diagonal (molecules moved rigidly with their oxygen's fractional coordinates)."""
    rng = np.random.default_rng(seed)
    confs = pos[None] + rng.normal(0.0, 0.003, size=(nconf,) + pos.shape)
    boxes = None if box is None else np.repeat(np.asarray(box, dtype=np.float64)[None], nconf, axis=0)
    if name == "w27s":
        s = rng.uniform(0.95, 1.05, size=(nconf, 3))
        confs = confs * s[:, None, :]
        boxes = boxes * s[:, None, :]
    if name == "mix":
        ortho = np.diag(np.diag(box))
        centres = confs[1][0::3]
        move = (centres @ np.linalg.inv(box)) @ ortho - centres
        confs[1] += np.repeat(move, 3, axis=0)
        boxes[1] = ortho
    confs[1::2] += SHIFT
    return np.ascontiguousarray(confs), None if boxes is None else np.ascontiguousarray(boxes)


def _cotangents(n, seed, nconf=B):
    """{set: (e_bar, f_bar)} -- E only, F only, both; seeded normal values."""
    rng = np.random.default_rng(seed)
    eb, fb = rng.normal(size=nconf), rng.normal(size=(nconf, n, 3))
    return {"E": (eb, None), "F": (None, fb), "EF": (eb, fb)}


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """(system, force, default box, conformations, boxes, cotangents)"""
    system, force, pos, box = _system(name)
    confs, boxes = _conformations(name, pos, box, 600 + SYSTEMS.index(name))
    if boxes is not None:
        for b in range(B):
            assert ljr.pair_gap_to_cutoff(force, confs[b], boxes[b]) > 1e-9
            assert all(force.getCutoffDistance() <= 0.5 * boxes[b][a, a] for a in range(3))
    if name == "mix":
        assert [b for b in range(B) if not (boxes[b][1, 0] or boxes[b][2, 0] or boxes[b][2, 1])] == [1]
    return system, force, box, confs, boxes, _cotangents(len(pos), 71 + SYSTEMS.index(name))


@functools.lru_cache(maxsize=None)
def _ref(name):
    """{set: (B, 2N)}: the numpy closed form, computed once per system and shared, read-only."""
    system, force, box, confs, boxes, cots = _inputs(name)
    out = {}
    for s, (eb, fb) in cots.items():
        rows = []
        for b in range(B):
            gs, ge = ljr.closed_form(force, confs[b], None if boxes is None else boxes[b],
                                     None if eb is None else eb[b], None if fb is None else fb[b])
            rows.append(np.concatenate([gs, ge]))
        out[s] = np.array(rows)
        if name != "c1+0":
            assert np.abs(out[s]).max() > 1.0, (name, s)
    return out


@functools.lru_cache(maxsize=None)
def _fd(name):
    """(checked parameters, checked conformations, {set: (len(checked), len(params))}): Richardson
    differences of the oracle, once per system."""
    system, force, box, confs, boxes, cots = _inputs(name)
    params = ljr.active_parameters(force)
    checked = list(range(B))
    if name in SAMPLED:
        rng = np.random.default_rng(9 + SYSTEMS.index(name))
        half = len(params) // 2
        params = sorted(int(p) for p in np.concatenate([rng.choice(params[:half], size=16, replace=False),
                                                        rng.choice(params[half:], size=16, replace=False)]))
        checked = [0]
    fd = ljr.richardson_fd(force, box, [confs[b] for b in checked],
                           None if boxes is None else [boxes[b] for b in checked],
                           {s: tuple(None if t is None else t[checked] for t in cot) for s, cot in cots.items()}, params)
    return params, checked, fd


def _kernel(name, **kw):
    system, force = _inputs(name)[:2]
    return HipCalcCoulForceKernel(**kw).initialize(system, force)


def _grad(k, confs, boxes, cot):
    return k.execute_batch_lj_vjp_host(confs, *cot, boxes=boxes)["flat"]


def _report(tag, err, scale):
    ratio = f"{err / scale:.3e}" if scale > 0 else "-"
    print(f"{tag}: max|grad - ref| = {err:.3e}, max|grad| = {scale:.3e}, ratio = {ratio}")


# 1, 3 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SYSTEMS)
def test_matches_the_closed_form(name):
    system, force, box, confs, boxes, cots = _inputs(name)
    ref = _ref(name)
    k = _kernel(name)
    n = confs.shape[1]
    off = [i for i in range(n) if force._eps[i] == 0.0]
    for s in SETS:
        out = k.execute_batch_lj_vjp_host(confs, *cots[s], boxes=boxes)
        g = out["flat"]
        assert g.shape == (B, 2 * n) and np.isfinite(g).all()
        assert out["sigmas"].shape == (B, n) and out["epsilons"].shape == (B, n)
        assert np.shares_memory(out["sigmas"], g) and np.shares_memory(out["epsilons"], g)
        assert np.array_equal(out["sigmas"], g[:, :n]) and np.array_equal(out["epsilons"], g[:, n:])
        err, scale = np.abs(g - ref[s]).max(), np.abs(g).max()
        _report(f"{name} [{s}] closed form", err, scale)
        assert err <= REL * scale + ABS, (name, s, err, scale)
        # an atom with eps = 0: exactly 0 for both
        assert np.array_equal(out["sigmas"][:, off], np.zeros((B, len(off))))
        assert np.array_equal(out["epsilons"][:, off], np.zeros((B, len(off))))
        if name == "c1+0":   # every pair excluded
            assert np.array_equal(g, np.zeros_like(g))
    if name == "c21+7v":
        assert force._sigma[63] == 0.0 and force._eps[63] > 0 and force._eps[64] == 0.0 and force._sigma[64] > 0
        g = _grad(k, confs, boxes, cots["EF"])
        assert np.abs(g[:, 63]).min() > 0 and np.abs(g[:, n + 63]).min() > 0   # sigma = 0: legal, and it interacts
    assert k.device_errors() == 0


# 2 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [s for s in SYSTEMS if s != "c1+0"])
def test_matches_extrapolated_differences_of_the_oracle(name):
    system, force, box, confs, boxes, cots = _inputs(name)
    params, checked, fd = _fd(name)
    if name in SAMPLED:
        n = confs.shape[1]
        assert len(params) == 32 and sum(p < n for p in params) == 16 and checked == [0]
    else:
        assert len(params) == 2 * sum(e > 0 for e in force._eps) and checked == list(range(B))
    k = _kernel(name)
    for s in SETS:
        g = _grad(k, confs, boxes, cots[s])
        err, scale = np.abs(g[checked][:, params] - fd[s]).max(), np.abs(g[checked]).max()
        _report(f"{name} [{s}] oracle differences", err, scale)
        assert scale > 1.0
        assert err <= REL * scale + ABS, (name, s, err, scale)


# 4 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c21+7", "c100+21", "w27s", "mix"])
def test_linearity_and_null_cotangents(name):
    system, force, box, confs, boxes, cots = _inputs(name)
    k = _kernel(name)
    n = confs.shape[1]
    g = {s: _grad(k, confs, boxes, cots[s]) for s in SETS}
    d = np.abs(g["EF"] - (g["E"] + g["F"])).max()
    print(f"{name}: linearity max|d| = {d:.3e}, max|grad| = {np.abs(g['EF']).max():.3e}")
    assert d <= 1e-12 * np.abs(g["EF"]).max()
    # no cotangent: exact zeros, whatever the array held; a call, its conformations, no pass
    stats = k.batch_stats()
    assert np.array_equal(_grad(k, confs, boxes, (None, None)), np.zeros((B, 2 * n)))
    pt = torch.tensor(confs, device="cuda:0")
    gt = torch.full((B, 2 * n), 7.0, dtype=torch.float64, device="cuda:0")
    k.execute_batch_lj_vjp_device(pt, gt, boxes=boxes)
    k.synchronize()
    assert (gt == 0.0).all()
    assert k.batch_stats() == (stats[0] + 2, stats[1] + 2 * B, stats[2])


# 5 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c2+1", "c100+21", "w27s", "mix", "w100"])
def test_bitwise_guarantees(name):
    stream = torch.cuda.Stream()
    system, force, box, confs, boxes, cots = _inputs(name)
    k = _kernel(name, stream=stream.cuda_stream)
    bx = lambda sel: None if boxes is None else np.ascontiguousarray(boxes[sel])
    for s in ("E", "EF"):
        cot = cots[s]
        c0, n0, p0 = k.batch_stats()
        g = _grad(k, confs, boxes, cot)
        assert k.batch_stats() == (c0 + 1, n0 + B, p0 + 1)      # one pass under the automatic limit
        assert np.array_equal(_grad(k, confs, boxes, cot), g)
        for b in range(B):                                      # alone (B = 1) = its row of the batch
            one = [None if t is None else np.ascontiguousarray(t[b:b + 1]) for t in cot]
            gb = _grad(k, np.ascontiguousarray(confs[b:b + 1]), bx(slice(b, b + 1)), one)
            assert np.array_equal(gb[0], g[b])
        rev = [None if t is None else np.ascontiguousarray(t[::-1]) for t in cot]
        gr = _grad(k, np.ascontiguousarray(confs[::-1]), bx(slice(None, None, -1)), rev)
        assert np.array_equal(gr[::-1], g)
        for limit, passes in ((1, 3), (2, 2)):
            p1 = k.batch_stats()[2]
            k.set_batch_limit(limit)
            g2 = _grad(k, confs, boxes, cot)
            assert k.batch_stats()[2] == p1 + passes
            assert np.array_equal(g2, g)
        k.set_batch_limit(0)
        # the device form on the side stream
        dev = lambda a: None if a is None else torch.tensor(a, device="cuda:0")
        pt, ct = dev(confs), [dev(t) for t in cot]
        gt = torch.full(g.shape, -3.0, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()   # the inputs exist before the side stream reads them
        own = None if boxes is None else boxes.copy()
        k.execute_batch_lj_vjp_device(pt, gt, *ct, boxes=own)
        if own is not None:
            own[:] = np.nan        # the boxes are the caller's again as soon as the call returns
        stream.synchronize()
        assert np.array_equal(gt.cpu().numpy(), g)
    assert k.device_errors() == 0


# 6 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c21+7", "w27s"])
def test_parameter_update_reaches_the_gradient_path(name):
    system, force, box, confs, boxes, cots = _inputs(name)
    force = copy.deepcopy(force)
    k = HipCalcCoulForceKernel().initialize(system, force)
    g0 = _grad(k, confs, boxes, cots["EF"])
    rng = np.random.default_rng(3)
    for i in range(force.getNumParticles()):
        q, s, e = force.getParticleParameters(i)
        force.setParticleParameters(i, q, s * (1 + 0.03 * rng.uniform(-1, 1)), e * (1 + 0.1 * rng.uniform(-1, 1)))
    k.copyParametersToContext(force)
    g1 = _grad(k, confs, boxes, cots["EF"])
    assert np.abs(g1 - g0).max() > 1e-3 * np.abs(g0).max()   # the update took effect
    fresh = HipCalcCoulForceKernel().initialize(system, force)
    assert np.array_equal(_grad(fresh, confs, boxes, cots["EF"]), g1)


# 7 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c21+7", "w100"])
def test_isolation_from_the_single_evaluation_state(name):
    system, force, box, confs, boxes, cots = _inputs(name)
    k = _kernel(name)
    box0 = None if boxes is None else boxes[0]
    e0, f0 = k.execute_host(confs[0], box0)
    diag = (k.charges(), k.energy_terms(), k.neighbor_stats())
    stats = k.batch_stats()
    g = _grad(k, confs, boxes, cots["EF"])
    assert k.batch_stats() == (stats[0] + 1, stats[1] + B, stats[2] + 1)
    after = (k.charges(), k.energy_terms(), k.neighbor_stats())
    assert np.array_equal(diag[0], after[0]) and np.array_equal(diag[1], after[1]) and diag[2] == after[2]
    e1, f1 = k.execute_host(confs[0], box0)
    assert e1 == e0 and np.array_equal(f1, f0)
    # the other batch calls in between leave it alone, and it them
    fw = k.execute_batch_host(confs, boxes=boxes)
    assert np.array_equal(_grad(k, confs, boxes, cots["EF"]), g)
    fw2 = k.execute_batch_host(confs, boxes=boxes)
    assert all(np.array_equal(a, b) for a, b in zip(fw, fw2))
    assert k.device_errors() == 0


# 8 ------------------------------------------------------------------------------------------
def test_argument_errors():
    lib = _cabi.load_library()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    vjp, vjp_host = lib.cf_compute_batch_lj_vjp, lib.cf_compute_batch_lj_vjp_host
    # a non-periodic handle with boxes
    system, force, box, confs, boxes, cots = _inputs("c2+1")
    kn = _kernel("c2+1")
    n = confs.shape[1]
    with pytest.raises(ChargeFluxError) as ei:
        kn.execute_batch_lj_vjp_host(confs, energy_bar=np.ones(B), boxes=np.diag([3.0, 3.0, 3.0]))
    assert ei.value.code == _cabi.CF_ERR_INVALID and "not periodic" in str(ei.value)
    assert kn.batch_stats() == (0, 0, 0)
    # nconf = 0, negative nconf, null positions, null grad; between begin and end
    pt = torch.tensor(confs, device="cuda:0")
    eb = torch.ones(B, dtype=torch.float64, device="cuda:0")
    gt = torch.full((B, 2 * n), 2.0, dtype=torch.float64, device="cuda:0")
    assert vjp(kn._h, 0, ptr(pt), None, ptr(eb), None, ptr(gt)) == _cabi.CF_OK
    assert vjp(kn._h, -1, ptr(pt), None, ptr(eb), None, ptr(gt)) == _cabi.CF_ERR_INVALID
    assert vjp(kn._h, B, None, None, ptr(eb), None, ptr(gt)) == _cabi.CF_ERR_INVALID
    assert vjp(kn._h, B, ptr(pt), None, ptr(eb), None, None) == _cabi.CF_ERR_INVALID
    assert vjp_host(kn._h, B, None, None, None, None, None) == _cabi.CF_ERR_INVALID
    assert kn.execute_batch_lj_vjp_host(np.zeros((0, n, 3)))["flat"].shape == (0, 2 * n)
    kn.begin(pt[0])
    with pytest.raises(ChargeFluxError) as ei:
        kn.execute_batch_lj_vjp_device(pt, gt, eb)
    assert ei.value.code == _cabi.CF_ERR_STATE
    kn.end()
    kn.synchronize()
    assert (gt == 2.0).all() and kn.batch_stats() == (0, 0, 0)
    k2 = HipCalcCoulForceKernel(rank=0, world_size=2).initialize(system, force)
    with pytest.raises(ChargeFluxError) as ei:
        k2.execute_batch_lj_vjp_host(confs, energy_bar=np.ones(B))
    assert ei.value.code == _cabi.CF_ERR_STATE
    # a periodic handle without boxes
    system, force, box, confs, boxes, cots = _inputs("w27s")
    k = _kernel("w27s")
    n = confs.shape[1]
    g = _grad(k, confs, boxes, cots["EF"])
    stats = k.batch_stats()
    pt = torch.tensor(confs, device="cuda:0")
    gt = torch.full((B, 2 * n), 2.0, dtype=torch.float64, device="cuda:0")

    def untouched():
        k.synchronize()
        return bool((gt == 2.0).all()) and k.batch_stats() == stats

    with pytest.raises(ChargeFluxError) as ei:
        k.execute_batch_lj_vjp_device(pt, gt, eb)
    assert ei.value.code == _cabi.CF_ERR_INVALID
    with pytest.raises(ChargeFluxError) as ei:
        k.execute_batch_lj_vjp_host(confs, energy_bar=np.ones(B))
    assert ei.value.code == _cabi.CF_ERR_INVALID
    assert untouched()
    # a bad box (cutoff above half a diagonal) in conformation 1: names it, touches nothing, counts nothing
    bad = boxes.copy()
    bad[1] = np.diag([0.9, 0.79, 0.9])                     # cutoff 0.4 > 0.395
    with pytest.raises(ChargeFluxError) as ei:
        k.execute_batch_lj_vjp_device(pt, gt, eb, boxes=bad)
    assert ei.value.code == _cabi.CF_ERR_INVALID and "conformation 1" in str(ei.value)
    assert untouched()
    with pytest.raises(ChargeFluxError) as ei:
        k.execute_batch_lj_vjp_host(confs, energy_bar=np.ones(B), boxes=bad)
    assert ei.value.code == _cabi.CF_ERR_INVALID and "conformation 1" in str(ei.value)
    assert untouched()
    # the call still works after all that, with the same bits
    assert np.array_equal(_grad(k, confs, boxes, cots["EF"]), g)
    assert k.device_errors() == 0


# 9 ------------------------------------------------------------------------------------------
def _model(name, nconf, seed):
    from openmmcoul.fitting import BatchedChargeFlux
    system, force, pos, box = _system(name)
    force = copy.deepcopy(force)
    k = HipCalcCoulForceKernel().initialize(system, force)
    rng = np.random.default_rng(seed)
    confs = np.ascontiguousarray(pos[None] + rng.normal(0.0, 0.003, size=(nconf,) + pos.shape))
    boxes = None if box is None else np.ascontiguousarray(np.repeat(np.asarray(box)[None], nconf, axis=0))
    return BatchedChargeFlux(k, force), torch.tensor(confs, device="cuda:0"), boxes


@pytest.mark.parametrize("name", ["c2+1", "w8"])
def test_autograd_gradcheck_over_the_active_lj_parameters(name):
    model, pos, boxes = _model(name, 2, 3)
    q, bonds, angles, waters = (p.detach() for p in model.parameters(device="cuda:0"))
    s0, e0 = (p.detach() for p in model.lj_parameters(device="cuda:0"))
    idx = torch.nonzero(e0 > 0).flatten()
    assert 0 < len(idx) < len(e0)
    s_act = s0[idx].clone().requires_grad_(True)
    e_act = e0[idx].clone().requires_grad_(True)

    def fn(sa, ea):   # a leaf of the active entries scattered into the full vector
        return model(q, bonds, angles, waters, pos, boxes=boxes, sigmas=s0.index_put((idx,), sa),
                     epsilons=e0.index_put((idx,), ea))

    assert torch.autograd.gradcheck(fn, (s_act, e_act), eps=1e-6, atol=1e-6, rtol=1e-6)


@pytest.mark.parametrize("name", ["c2+1", "w8"])
def test_without_lj_tensors_the_path_is_the_old_one(name):
    model, pos, boxes = _model(name, 2, 4)
    untouched, pos2, _ = _model(name, 2, 4)
    params = model.parameters(device="cuda:0")
    lj = model.lj_parameters(device="cuda:0")
    with_lj = model(*params, pos, boxes=boxes, sigmas=lj[0], epsilons=lj[1])
    stats = model.kernel.batch_stats()
    out = model(*params, pos, boxes=boxes)
    ref = untouched(*untouched.parameters(device="cuda:0"), pos2, boxes=boxes)
    assert all(torch.equal(a, b) for a, b in zip(out, ref))
    assert all(torch.equal(a, b) for a, b in zip(with_lj, ref))   # the force's own sigma / epsilon, given back
    out[1].square().sum().backward()
    assert model.kernel.batch_stats()[0] == stats[0] + 2            # the forward and one VJP: no extra call
    grads = [p.grad.clone() for p in params]
    rparams = untouched.parameters(device="cuda:0")
    untouched(*rparams, pos2, boxes=boxes)[1].square().sum().backward()
    assert all(torch.equal(a, p.grad) for a, p in zip(grads, rparams))
    # only the LJ tensors need grad: one LJ call, the other VJP skipped
    frozen = [p.detach() for p in params]
    stats = model.kernel.batch_stats()
    model(*frozen, pos, boxes=boxes, sigmas=lj[0], epsilons=lj[1])[1].square().sum().backward()
    assert model.kernel.batch_stats()[0] == stats[0] + 2
    assert lj[0].grad is not None and lj[1].grad is not None and lj[0].grad.abs().max() > 0
    off = torch.nonzero(lj[1].detach() == 0).flatten()
    assert (lj[0].grad[off] == 0).all() and (lj[1].grad[off] == 0).all()


@pytest.mark.parametrize("name", ["c2+1", "w8"])
def test_adam_lowers_a_force_matching_loss_over_all_six_tensors(name):
    model, pos, boxes = _model(name, 2, 9)
    start = [p.detach().clone() for p in model.parameters(device="cuda:0") + model.lj_parameters(device="cuda:0")]
    rng = np.random.default_rng(1)
    call = lambda p: model(*p[:4], pos, boxes=boxes, sigmas=p[4], epsilons=p[5])
    with torch.no_grad():
        truth = [p * torch.tensor(1 + 0.05 * rng.uniform(-1, 1, size=tuple(p.shape)), device=p.device) for p in start]
        target = call(truth)[1]
    params = [p.clone().requires_grad_(True) for p in start]
    opt = torch.optim.Adam(params, lr=1e-4)
    losses = []
    for _ in range(4):
        opt.zero_grad()
        loss = ((call(params)[1] - target) ** 2).mean()
        losses.append(loss.item())
        loss.backward()
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in params)
        opt.step()
    print("force-matching loss:", " ".join(f"{v:.6e}" for v in losses))
    assert losses[1] < losses[0] and losses[2] < losses[1] and losses[3] < losses[2]
    assert torch.equal(params[5].detach() == 0, start[5] == 0)   # an atom without LJ stays without
