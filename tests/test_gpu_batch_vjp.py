"""GPU tests of the parameter gradients of the non-periodic batch (cf_compute_batch_vjp,
include/chargeflux.h; DESIGN.md "Batched, parameter gradients"): against central differences of the
oracle, a term with k = 0, linearity in the cotangents and the NULL cases, the bitwise guarantees,
isolation from the single-evaluation state, parameter updates, the argument errors and the torch
autograd layer (openmmcoul.fitting).

Systems: the `_cluster` recipe of test_gpu_batch.py (C1's recipe), B = 3 conformations.

The scalar differentiated per conformation is L = e_bar E + q_bar . q + F_bar . F.  L is exactly
quadratic in every single parameter, so a central difference along one parameter has no truncation
error, only round-off ~ eps |L| / h: h = 1e-2 in the parameter's own unit.

Bar (every finite-difference comparison here):  max |grad - fd| <= 1e-9 max |grad| + 1e-9, the maxima
taken per system and cotangent set over the checked conformations (max |grad| over all of their
parameters).  Observed on MI355X (printed by the tests): see DESIGN.md.
"""
import copy
import ctypes as C
import functools
import math

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
SHIFT = np.array([0.4, -0.2, 0.1])
SETS = ("E", "q", "F", "EqF")
# (waters, ions): every pair excluded; no terms (P = N); small; across one wave; across a 256 tile
# with a tail; C1
FULL_SIZES = [(1, 0), (0, 5), (2, 1), (21, 7)]
SAMPLED_SIZES = [(100, 21), (64, 64)]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _cluster(nw, ni, seed=ts.SEED):
    if (nw, ni) == (64, 64):
        system, force, pos, _ = ts.cluster_c1()
        return system, force, pos
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


def _conformations(pos, seed):
    """B conformations: base + N(0, 0.003 nm) per coordinate; the odd ones also translated."""
    rng = np.random.default_rng(seed)
    confs = pos[None] + rng.normal(0.0, 0.003, size=(B,) + pos.shape)
    confs[1::2] += SHIFT
    return np.ascontiguousarray(confs)


def _cotangents(n, seed):
    """{set: (e_bar, q_bar, f_bar)} -- E only, q only, F only, all three; seeded normal values."""
    rng = np.random.default_rng(seed)
    eb, qb, fb = rng.normal(size=B), rng.normal(size=(B, n)), rng.normal(size=(B, n, 3))
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


def _fd(force, confs, cots, params, nconf):
    """Central differences of the oracle: {set: (nconf, len(params))}.  One oracle per perturbed
    force, shared by the conformations and the cotangent sets."""
    out = {s: np.zeros((nconf, len(params))) for s in SETS}
    for col, p in enumerate(params):
        res = []
        for sign in (1.0, -1.0):
            o = Oracle(_perturbed(force, p, sign * H_FD))
            res.append([o.execute(confs[b], None) for b in range(nconf)])
        for s in SETS:
            for b in range(nconf):
                out[s][b, col] = (_loss(res[0][b], cots[s], b) - _loss(res[1][b], cots[s], b)) / (2 * H_FD)
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
def _case(nw, ni):
    """(system, force, conformations, cotangents, checked parameters, checked conformations, fd):
    the finite differences run once per system and are shared, read-only."""
    system, force, pos = _cluster(nw, ni)
    confs = _conformations(pos, 177 + nw + ni)
    cots = _cotangents(pos.shape[0], 31 + nw + ni)
    if (nw, ni) in SAMPLED_SIZES:
        params, nconf = _sample(force, 5 + nw + ni), 1
    else:
        params, nconf = list(range(sum(_counts(force)))), B
    return system, force, confs, cots, params, nconf, _fd(force, confs, cots, params, nconf)


def _kernel(nw, ni, **kw):
    system, force = _case(nw, ni)[:2]
    return HipCalcCoulForceKernel(**kw).initialize(system, force)


def _check_against_fd(tag, k, confs, cots, params, nconf, fd):
    for s in SETS:
        g = k.execute_batch_vjp_host(confs, *cots[s])["flat"]
        assert np.isfinite(g).all()
        err = np.abs(g[:nconf][:, params] - fd[s]).max()
        scale = np.abs(g[:nconf]).max()
        ratio = f"{err / scale:.3e}" if scale > 0 else "-"
        print(f"{tag} [{s}]: max|grad - fd| = {err:.3e}, max|grad| = {scale:.3e}, ratio = {ratio}")
        assert err <= REL * scale + ABS, (tag, s, err, scale)


# 1 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nw,ni", FULL_SIZES + SAMPLED_SIZES)
def test_matches_central_differences_of_the_oracle(nw, ni):
    system, force, confs, cots, params, nconf, fd = _case(nw, ni)
    k = _kernel(nw, ni)
    assert k.param_counts() == _counts(force)
    if (nw, ni) in SAMPLED_SIZES:
        counts = _counts(force)
        edges = np.cumsum((0,) + counts)
        for kind in range(4):
            if counts[kind]:
                assert sum(edges[kind] <= p < edges[kind + 1] for p in params) >= 8
        assert len(params) == 64
    _check_against_fd(f"{nw}+{ni}", k, confs, cots, params, nconf, fd)
    if (nw, ni) == (1, 0):   # every pair excluded: nothing depends on the parameters through E or F
        for s in ("E", "F"):
            g = k.execute_batch_vjp_host(confs, *cots[s])["flat"]
            assert np.array_equal(g, np.zeros_like(g))


# 2 ------------------------------------------------------------------------------------------
def test_a_term_with_k_zero():
    system, force, pos = _cluster(21, 7)
    force = copy.deepcopy(force)
    force._fbond_par[0] = (0.0, force._fbond_par[0][1])
    force._fangle_par[0] = (0.0, force._fangle_par[0][1])
    k1, k2, kub, b0, ub0 = force._fwater_par[0]
    force._fwater_par[0] = (0.0, 0.0, 0.0, b0, ub0)
    confs = _conformations(pos, 19)
    cots = _cotangents(pos.shape[0], 23)
    params = list(range(sum(_counts(force))))
    k = HipCalcCoulForceKernel().initialize(system, force)
    _check_against_fd("21+7, k = 0", k, confs, cots, params, 1, _fd(force, confs, cots, params, 1))


# 3 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nw,ni", [(21, 7), (100, 21)])
def test_linearity_and_null_cotangents(nw, ni):
    system, force, confs, cots = _case(nw, ni)[:4]
    k = _kernel(nw, ni)
    g = {s: k.execute_batch_vjp_host(confs, *cots[s])["flat"] for s in SETS}
    total = g["E"] + g["q"] + g["F"]
    d = np.abs(g["EqF"] - total).max()
    print(f"{nw}+{ni}: linearity max|d| = {d:.3e}, max|grad| = {np.abs(g['EqF']).max():.3e}")
    assert d <= 1e-12 * np.abs(g["EqF"]).max()
    # no cotangent: exact zeros, whatever the array held
    out = k.execute_batch_vjp_host(confs)
    assert np.array_equal(out["flat"], np.zeros((B, sum(_counts(force)))))
    n = confs.shape[1]
    pt = torch.tensor(confs, device="cuda:0")
    gt = torch.full((B, sum(_counts(force))), 7.0, dtype=torch.float64, device="cuda:0")
    k.execute_batch_vjp_device(pt, gt)
    k.synchronize()
    assert (gt == 0.0).all()
    # the views
    assert out["charges"].shape == (B, n) and out["bonds"].shape == (B, force.getNumFluxBonds(), 2)
    assert out["angles"].shape == (B, force.getNumFluxAngles(), 2)
    assert out["waters"].shape == (B, force.getNumFluxWaters(), 5)
    assert all(np.shares_memory(out[key], out["flat"]) for key in ("charges", "bonds", "angles", "waters"))
    # e_bar = 1 alone: the charges block is dE/dq
    ge = k.execute_batch_vjp_host(confs, energy_bar=np.ones(B))
    for b in range(B):
        k.execute_host(confs[b])
        dedq = k.dedq()
        assert np.abs(ge["charges"][b] - dedq).max() <= 1e-12 * np.abs(dedq).max() + 1e-10


# 4 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nw,ni", [(2, 1), (100, 21), (64, 64)])
def test_bitwise_guarantees(nw, ni):
    system, force, confs, cots = _case(nw, ni)[:4]
    k = _kernel(nw, ni)
    for s in ("E", "EqF"):
        cot = cots[s]
        c0, n0, p0 = k.batch_stats()
        g = k.execute_batch_vjp_host(confs, *cot)["flat"]
        assert k.batch_stats() == (c0 + 1, n0 + B, p0 + 1)      # one pass under the automatic limit
        assert np.array_equal(k.execute_batch_vjp_host(confs, *cot)["flat"], g)
        for b in range(B):                                      # alone (B = 1) = its row of the batch
            one = [None if t is None else np.ascontiguousarray(t[b:b + 1]) for t in cot]
            gb = k.execute_batch_vjp_host(np.ascontiguousarray(confs[b:b + 1]), *one)["flat"]
            assert np.array_equal(gb[0], g[b])
        rev = [None if t is None else np.ascontiguousarray(t[::-1]) for t in cot]
        gr = k.execute_batch_vjp_host(np.ascontiguousarray(confs[::-1]), *rev)["flat"]
        assert np.array_equal(gr[::-1], g)
        p1 = k.batch_stats()[2]
        k.set_batch_limit(2)
        g2 = k.execute_batch_vjp_host(confs, *cot)["flat"]
        assert k.batch_stats()[2] == p1 + 2                     # 2 + 1 conformations
        assert np.array_equal(g2, g)
        k.set_batch_limit(0)


def test_device_form_on_a_side_stream_equals_host_form():
    stream = torch.cuda.Stream()
    system, force, confs, cots = _case(100, 21)[:4]
    k = _kernel(100, 21, stream=stream.cuda_stream)
    g = k.execute_batch_vjp_host(confs, *cots["EqF"])["flat"]
    dev = lambda a: torch.tensor(a, device="cuda:0")
    pt, (eb, qb, fb) = dev(confs), [dev(t) for t in cots["EqF"]]
    gt = torch.full(g.shape, -3.0, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()   # the inputs exist before the side stream reads them
    k.execute_batch_vjp_device(pt, gt, eb, qb, fb)
    stream.synchronize()
    assert np.array_equal(gt.cpu().numpy(), g)
    views = k.split_gradient(gt, k.param_counts())
    assert views["waters"].shape == (B, force.getNumFluxWaters(), 5)


# 5 ------------------------------------------------------------------------------------------
def test_isolation_from_the_single_evaluation_state():
    system, force, confs, cots = _case(64, 64)[:4]
    k = _kernel(64, 64)
    k.set_graph(True)
    e0, f0 = k.execute_host(confs[0])
    e0, f0 = k.execute_host(confs[0])
    diag = (k.charges(), k.dedq(), k.energy_terms(), k.neighbor_stats(), k.graph_stats())
    stats = k.batch_stats()
    g = k.execute_batch_vjp_host(confs, *cots["EqF"])["flat"]
    assert k.batch_stats() == (stats[0] + 1, stats[1] + B, stats[2] + 1)
    after = (k.charges(), k.dedq(), k.energy_terms(), k.neighbor_stats(), k.graph_stats())
    for a, b in zip(diag[:3], after[:3]):
        assert np.array_equal(a, b)
    assert diag[3:] == after[3:]
    e1, f1 = k.execute_host(confs[0])
    assert e1 == e0 and np.array_equal(f1, f0)
    # the forward batch and the gradients share a workspace: neither disturbs the other
    e, f, q = k.execute_batch_host(confs)
    assert np.array_equal(k.execute_batch_vjp_host(confs, *cots["EqF"])["flat"], g)
    e2, f2, q2 = k.execute_batch_host(confs)
    assert np.array_equal(e, e2) and np.array_equal(f, f2) and np.array_equal(q, q2)


# 6 ------------------------------------------------------------------------------------------
def test_parameter_update_reaches_the_gradient_path():
    system, force, pos = _cluster(21, 7, seed=5)
    force = copy.deepcopy(force)
    confs = _conformations(pos, 11)
    cots = _cotangents(pos.shape[0], 13)
    k = HipCalcCoulForceKernel().initialize(system, force)
    g0 = k.execute_batch_vjp_host(confs, *cots["EqF"])["flat"]
    for i in range(force.getNumParticles()):
        q, s, e = force.getParticleParameters(i)
        force.setParticleParameters(i, q * 1.05, s, e)
    for w in range(force.getNumFluxWaters()):
        k1, k2, kub, b0, ub0 = force._fwater_par[w]
        force._fwater_par[w] = (k1 * 1.1, k2, kub, b0, ub0)
    k.copyParametersToContext(force)
    g1 = k.execute_batch_vjp_host(confs, *cots["EqF"])["flat"]
    assert np.abs(g1 - g0).max() > 1e-3 * np.abs(g0).max()   # the update took effect
    params = list(range(sum(_counts(force))))
    _check_against_fd("21+7, updated", k, confs, cots, params, 1, _fd(force, confs, cots, params, 1))


# 7 ------------------------------------------------------------------------------------------
def test_argument_errors():
    lib = _cabi.load_library()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    # periodic handle
    system, force, pos, box = ts.water_box(100, cutoff=0.6)
    kp = HipCalcCoulForceKernel().initialize(system, force)
    with pytest.raises(ChargeFluxError) as ei:
        kp.execute_batch_vjp_host(np.ascontiguousarray(pos[None]), energy_bar=np.ones(1))
    assert ei.value.code == _cabi.CF_ERR_INVALID and "non-periodic" in str(ei.value)
    # nconf = 0: OK, nothing written, nothing counted
    system, force, confs, cots = _case(0, 5)[:4]
    k = _kernel(0, 5)
    n = confs.shape[1]
    pt = torch.tensor(confs, device="cuda:0")
    eb = torch.ones(B, dtype=torch.float64, device="cuda:0")
    gt = torch.full((B, n), 2.0, dtype=torch.float64, device="cuda:0")
    stats = k.batch_stats()
    assert lib.cf_compute_batch_vjp(k._h, 0, ptr(pt), ptr(eb), None, None, ptr(gt)) == _cabi.CF_OK
    k.synchronize()
    assert k.batch_stats() == stats
    assert (gt == 2.0).all()
    assert k.execute_batch_vjp_host(np.zeros((0, n, 3)))["flat"].shape == (0, n)
    # negative nconf, null positions, null grad
    assert lib.cf_compute_batch_vjp(k._h, -1, ptr(pt), ptr(eb), None, None, ptr(gt)) == _cabi.CF_ERR_INVALID
    assert lib.cf_compute_batch_vjp(k._h, B, None, ptr(eb), None, None, ptr(gt)) == _cabi.CF_ERR_INVALID
    assert lib.cf_compute_batch_vjp(k._h, B, ptr(pt), ptr(eb), None, None, None) == _cabi.CF_ERR_INVALID
    assert lib.cf_compute_batch_vjp_host(k._h, B, None, None, None, None, None) == _cabi.CF_ERR_INVALID
    k.synchronize()
    assert (gt == 2.0).all() and k.batch_stats() == stats
    # between cf_compute_begin and _end
    k.begin(pt[0])
    with pytest.raises(ChargeFluxError) as ei:
        k.execute_batch_vjp_device(pt, gt, eb)
    assert ei.value.code == _cabi.CF_ERR_STATE
    k.end()
    k.synchronize()
    # several ranks
    system, force, confs2 = _case(64, 64)[:3]
    k2 = HipCalcCoulForceKernel(rank=0, world_size=2).initialize(system, force)
    with pytest.raises(ChargeFluxError) as ei:
        k2.execute_batch_vjp_host(confs2, energy_bar=np.ones(B))
    assert ei.value.code == _cabi.CF_ERR_STATE


# 8 ------------------------------------------------------------------------------------------
def _model(nw, ni, nconf, seed):
    from openmmcoul.fitting import BatchedChargeFlux
    system, force, pos = _cluster(nw, ni)
    force = copy.deepcopy(force)
    k = HipCalcCoulForceKernel().initialize(system, force)
    rng = np.random.default_rng(seed)
    confs = pos[None] + rng.normal(0.0, 0.003, size=(nconf,) + pos.shape)
    return BatchedChargeFlux(k, force), torch.tensor(confs, device="cuda:0")


def test_autograd_gradcheck():
    model, pos = _model(2, 1, 2, 3)
    params = model.parameters(device="cuda:0")
    assert [tuple(p.shape) for p in params] == [(7,), (2, 2), (1, 2), (1, 5)]
    fn = lambda q, b, a, w: model(q, b, a, w, pos)
    assert torch.autograd.gradcheck(fn, params, eps=1e-3, atol=1e-7, rtol=1e-7)
    with pytest.raises(ValueError):
        model(*params, pos.clone().requires_grad_(True))


def test_adam_lowers_a_force_matching_loss():
    model, pos = _model(21, 7, 4, 9)
    start = [p.detach().clone() for p in model.parameters(device="cuda:0")]
    rng = np.random.default_rng(1)
    with torch.no_grad():
        truth = [p * torch.tensor(1 + 0.05 * rng.uniform(-1, 1, size=tuple(p.shape)), device=p.device) for p in start]
        target = model(*truth, pos)[1]
    params = [p.clone().requires_grad_(True) for p in start]
    opt = torch.optim.Adam(params, lr=2e-4)
    losses = []
    for _ in range(4):
        opt.zero_grad()
        loss = ((model(*params, pos)[1] - target) ** 2).mean()
        losses.append(loss.item())
        loss.backward()
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in params)
        opt.step()
    print("force-matching loss:", " ".join(f"{v:.6e}" for v in losses))
    assert losses[1] < losses[0] and losses[2] < losses[1] and losses[3] < losses[2]
