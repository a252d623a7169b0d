"""GPU tests of cf_compute_batch_periodic_hvp_vjp (include/chargeflux.h; DESIGN.md "Batched, periodic,
Hessian-vector parameter gradients") against central differences of the periodic complex-step products
(tests/pbc_hvp_vjp_reference.py, guarded on the CPU by tests/test_batch_periodic_hvp_vjp_cpu.py).
Systems, boxes and conformations: the recipes of test_gpu_batch_periodic_vjp.py, B = 2 (conformations 0
and 1; in conformation 1 every fifth atom is moved by a whole box vector), seeded N(0, 1) directions
and cotangents.  Condition on the inputs (asserted, not a tolerance): no non-excluded minimum-image
pair within 1e-9 nm of the cutoff and no minimum-image component within 1e-9 nm of a face.
Bar: max|grad - ref| <= 1e-9 max|ref| + 1e-9 per parameter group; observed on MI355X: see DESIGN.md.

The per-parameter reference rows (B,K,P) of `w22` and `tric` cost 2 P complex-step force evaluations
per (conformation, direction), minutes in numpy, so they are recorded in
tests/golden/pbc_hvp_vjp_rows.npz: `_live_rows(name)` saved under the system's name.  The rows of `w1`
and `ions` are computed live, and test_recorded_rows_match_the_live_reference recomputes seeded
parameters of the recorded ones.
"""
import copy
import ctypes as C
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import Oracle  # noqa: E402
from openmmcoul import ChargeFluxError, HipCalcCoulForceKernel, _cabi  # noqa: E402
from openmmcoul import testsystems as ts  # noqa: E402
from openmmcoul.fitting import BatchedChargeFlux  # noqa: E402
from tests import hvp_vjp_reference as hvr  # noqa: E402
from tests import pbc_hvp_vjp_reference as pvr  # noqa: E402
from tests.test_gpu_batch_periodic_vjp import (SYSTEMS, _assert_clear_of_cutoff, _conformations, _counts,  # noqa: E402
                                               _min_image, _system)

B, KC = 2, 4   # KC: the direction rows a block of the pair and k-space kernels carries
K = KC + 1
REL, ABS = 1e-9, 1e-9
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pbc_hvp_vjp_rows.npz")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """(system, force, default box, conformations, boxes, directions, cotangents (B,K,N,3)); the input condition."""
    system, force, pos, box = _system(name)
    confs, boxes = (np.ascontiguousarray(a[:B]) for a in _conformations(name, pos, box, 400 + SYSTEMS.index(name)))
    for x, bb in zip(confs, boxes):
        _assert_clear_of_cutoff(force, x, bb)
        d = _min_image(x[None, :, :] - x[:, None, :], bb)[~np.eye(len(x), dtype=bool)]
        assert np.abs(np.abs(d) - 0.5 * np.diag(bb)).min() > 1e-9
    vec, ubar = np.random.default_rng(900 + SYSTEMS.index(name)).normal(size=(2, B, K) + pos.shape)
    return system, force, box, confs, boxes, vec, ubar


def _refs(force, box, boxes):
    ewald = Oracle(force, box).ewald()
    return [pvr.Reference(force, *ewald, bb) for bb in boxes]


def _reference_rows(force, box, confs, boxes, vec, ubar):
    return np.stack([hvr.grad_rows(r, x, v, u) for r, x, v, u in zip(_refs(force, box, boxes), confs, vec, ubar)])


def _rows_at(force, box, x, bb, v, u, params):
    """(len(params),): the reference gradient at the flat parameters `params`, summed over the directions."""
    ref = _refs(force, box, bb[None])[0]
    return np.array([hvr.directional(ref, x, v, u, e).sum() for e in np.eye(len(ref.theta))[params]])


def _live_rows(name):
    system, force, box, confs, boxes, vec, ubar = _inputs(name)
    return _reference_rows(force, box, confs, boxes, vec, ubar)   # (B,K,P)


@functools.lru_cache(maxsize=None)
def _rows(name):
    return np.load(GOLDEN)[name] if name in ("w22", "tric") else _live_rows(name)


def _kernel(name, **kw):
    system, force = _inputs(name)[:2]
    return HipCalcCoulForceKernel(**kw).initialize(system, force)


_check = functools.partial(hvr.check_groups, rel=REL, ab=ABS)


def _cut(a, nvec):
    return np.ascontiguousarray(a[:, :nvec])


@pytest.mark.parametrize("name", ["w22", "tric"])
def test_recorded_rows_match_the_live_reference(name):
    system, force, box, confs, boxes, vec, ubar = _inputs(name)
    rows = _rows(name)
    assert rows.shape == (B, K, sum(_counts(force)))
    picks = np.random.default_rng(5).choice(rows.shape[2], size=4, replace=False)
    live = _rows_at(force, box, confs[1], boxes[1], vec[1, 3:], ubar[1, 3:], picks)
    _check(name, rows[1, 3:][:, picks].sum(axis=0), live, (len(picks),))


@pytest.mark.parametrize("nvec", [1, KC, KC + 1])
@pytest.mark.parametrize("name", ["w1", "ions", "w22", "tric"])
def test_matches_the_reference_per_parameter(name, nvec):
    system, force, box, confs, boxes, vec, ubar = _inputs(name)
    k = _kernel(name)
    got = k.execute_batch_hvp_vjp_host(confs, _cut(vec, nvec), _cut(ubar, nvec), boxes=boxes)["flat"]
    _check(f"{name} K={nvec}", got, _rows(name)[:, :nvec].sum(axis=1), _counts(force))
    assert k.device_errors() == 0


@pytest.mark.parametrize("name", ["w100", "aniso"])
def test_matches_the_reference_along_parameter_directions(name):
    system, force, box, confs, boxes, vec, ubar = _inputs(name)
    confs, boxes, vec, ubar = confs[:1], boxes[:1], _cut(vec[:1], 2), _cut(ubar[:1], 2)
    ref = _refs(force, box, boxes)[0]
    dirs = hvr.seeded_directions(ref, 91, 3)
    want = np.array([hvr.directional(ref, confs[0], vec[0], ubar[0], d).sum() for d in dirs])
    got = _kernel(name).execute_batch_hvp_vjp_host(confs, vec, ubar, boxes=boxes)["flat"][0] @ dirs.T
    _check(f"{name} base and k-type", got[:3], want[:3], (3,))
    _check(f"{name} ref-type", got[3:], want[3:], (3,))


def test_symmetry_and_aliasing():
    system, force, box, confs, boxes, vec, ubar = _inputs("w22")
    k = _kernel("w22")
    g = k.execute_batch_hvp_vjp_host(confs, vec, ubar, boxes=boxes)["flat"]
    swapped = k.execute_batch_hvp_vjp_host(confs, ubar, vec, boxes=boxes)["flat"]
    print(f"w22: max|g(u,v) - g(v,u)| = {np.abs(g - swapped).max():.3e}, max|g| = {np.abs(g).max():.3e}")
    assert np.abs(g - swapped).max() <= 1e-12 * np.abs(g).max()
    assert np.array_equal(k.execute_batch_hvp_vjp_host(confs, vec, vec, boxes=boxes)["flat"],
                          k.execute_batch_hvp_vjp_host(confs, vec, vec.copy(), boxes=boxes)["flat"])


# zero directions that force a conformation's directions into several passes: more rows than the 256 MiB
# workspace holds at 6 khalf + 3 G + 7 N doubles each (khalf = 1098: 5060, 3496 and 4535 rows)
PAD = {"ions": 6000, "w100": 4096, "tric": 6000}


@pytest.mark.parametrize("name", ["ions", "w100", "tric"])
def test_bitwise_guarantees(name):
    system, force, box, confs, boxes, vec, ubar = _inputs(name)
    k = _kernel(name)
    run = lambda sel: k.execute_batch_hvp_vjp_host(*(np.ascontiguousarray(a[sel]) for a in (confs, vec, ubar)),
                                                   boxes=np.ascontiguousarray(boxes[sel]))["flat"]
    c0, n0, p0 = k.batch_stats()
    g = run(slice(None))
    assert k.batch_stats() == (c0 + 1, n0 + B, p0 + 1)          # one pass under the automatic limit
    assert np.array_equal(run(slice(None)), g)
    for b in range(B):                                          # alone = its row of the batch
        assert np.array_equal(run(slice(b, b + 1))[0], g[b])
    assert np.array_equal(run(slice(None, None, -1))[::-1], g)  # any position of the batch
    p1 = k.batch_stats()[2]
    k.set_batch_limit(1)
    assert np.array_equal(run(slice(None)), g) and k.batch_stats()[2] == p1 + B
    k.set_batch_limit(0)
    gt = torch.full(g.shape, float("nan"), dtype=torch.float64, device="cuda:0")   # grad is overwritten
    k.execute_batch_hvp_vjp_device(*(torch.tensor(a, device="cuda:0") for a in (confs, vec)), gt,
                                   torch.tensor(ubar, device="cuda:0"), boxes=boxes)
    k.synchronize()
    assert np.array_equal(gt.cpu().numpy(), g)
    # the directions split over passes: every term carries a factor from v, so the zero rows add exact
    # zeros to the running sums
    real = 3
    v = np.zeros((1, PAD[name] + real) + confs.shape[1:])
    u = np.random.default_rng(7).normal(size=v.shape)
    v[:, PAD[name]:], u[:, PAD[name]:] = vec[:1, :real], ubar[:1, :real]
    p2 = k.batch_stats()[2]
    split = k.execute_batch_hvp_vjp_host(confs[:1], v, u, boxes=boxes[:1])["flat"]
    assert k.batch_stats()[2] > p2 + 1
    assert np.array_equal(split, k.execute_batch_hvp_vjp_host(confs[:1], _cut(vec[:1], real), _cut(ubar[:1], real),
                                                              boxes=boxes[:1])["flat"])
    assert k.device_errors() == 0


def test_isolation_from_the_other_periodic_batches():
    system, force, box, confs, boxes, vec, ubar = _inputs("w22")
    k = _kernel("w22")
    fb = np.random.default_rng(3).normal(size=confs.shape)
    before = lambda: (k.execute_batch_hvp_host(confs, vec, boxes=boxes), *k.execute_batch_host(confs, boxes=boxes),
                      k.execute_batch_vjp_host(confs, forces_bar=fb, boxes=boxes)["flat"])
    old = before()
    k.execute_batch_hvp_vjp_host(confs, vec, ubar, boxes=boxes)
    assert all(np.array_equal(a, b) for a, b in zip(old, before()))


def test_k_zero_and_parameter_updates():
    """Against the reference at the parameters of the three k = 0 terms and at three base charges."""
    system, force, box, confs, boxes, vec, ubar = _inputs("w22")
    confs, boxes, vec, ubar = confs[1:], boxes[1:], _cut(vec[1:], 2), _cut(ubar[1:], 2)
    force = copy.deepcopy(force)
    n, nb, na, nw = _counts(force)
    params = np.r_[0, 1, 2, n, n + 1, n + nb, n + nb + 1, n + nb + na + np.arange(5)]
    want = lambda: _rows_at(force, box, confs[0], boxes[0], vec[0], ubar[0], params)
    force._fbond_par[0] = (0.0, force._fbond_par[0][1])
    force._fangle_par[0] = (0.0, force._fangle_par[0][1])
    force._fwater_par[0] = (0.0, 0.0, 0.0) + tuple(force._fwater_par[0][3:])
    k = HipCalcCoulForceKernel().initialize(system, force)
    g0 = k.execute_batch_hvp_vjp_host(confs, vec, ubar, boxes=boxes)["flat"]
    _check("w22, k = 0", g0[0, params], want(), (len(params),))
    for i in range(force.getNumParticles()):
        q, s, e = force.getParticleParameters(i)
        force.setParticleParameters(i, q * 1.05, s, e)
    force._fwater_par[0] = (-1.1, 0.2, 0.5) + tuple(force._fwater_par[0][3:])
    k.copyParametersToContext(force)
    g1 = k.execute_batch_hvp_vjp_host(confs, vec, ubar, boxes=boxes)["flat"]
    assert np.abs(g1 - g0).max() > 1e-3 * np.abs(g0).max()      # the update took effect
    _check("w22, updated", g1[0, params], want(), (len(params),))


def test_torch_layer():
    system, force, box, confs, boxes, vec, ubar = _inputs("w22")
    force = copy.deepcopy(force)
    k = HipCalcCoulForceKernel().initialize(system, force)
    model = BatchedChargeFlux(k, force)
    params = model.parameters()
    pt, vt, wt = (torch.tensor(a, device="cuda:0") for a in (confs, vec, ubar))
    out = model.hvp(*params, pt, vt, boxes=boxes)
    assert np.array_equal(out.detach().cpu().numpy(), k.execute_batch_hvp_host(confs, vec, boxes=boxes))
    (wt * out).sum().backward()
    want = k.execute_batch_hvp_vjp_host(confs, vec, ubar, boxes=boxes)
    for p, name in zip(params, ("charges", "bonds", "angles", "waters")):
        assert np.array_equal(p.grad.numpy(), torch.tensor(want[name]).sum(dim=0).numpy()), name


def test_argument_errors_and_counting():
    lib = _cabi.load_library()
    system, force, cpos, _ = ts.cluster_c1()             # a non-periodic handle with boxes
    kn = HipCalcCoulForceKernel().initialize(system, force)
    with pytest.raises(ChargeFluxError) as ei:
        kn.execute_batch_hvp_vjp_host(np.ascontiguousarray(cpos[None]), np.ones((1, 1) + cpos.shape), boxes=np.eye(3) * 3.0)
    assert ei.value.code == _cabi.CF_ERR_INVALID and "periodic" in str(ei.value)
    system, force, box, confs, boxes, vec, ubar = _inputs("w22")
    k = _kernel("w22")
    n, npar = confs.shape[1], sum(k.param_counts())
    pt, vt, ut = (torch.tensor(a, device="cuda:0") for a in (confs, vec, ubar))
    gt = torch.full((B, npar), float("nan"), dtype=torch.float64, device="cuda:0")
    k.execute_batch_hvp_vjp_device(pt, vt, gt, ut, boxes=boxes)   # grad is overwritten, not added to
    k.synchronize()
    assert np.array_equal(gt.cpu().numpy(), k.execute_batch_hvp_vjp_host(confs, vec, ubar, boxes=boxes)["flat"])
    stats = k.batch_stats()
    for zero in (k.execute_batch_hvp_vjp_host(confs, vec, boxes=boxes)["flat"],                          # out_bar = None
                 k.execute_batch_hvp_vjp_host(confs, *np.zeros((2, B, 0, n, 3)), boxes=boxes)["flat"]):  # the empty sum
        assert zero.shape == gt.shape and not zero.any()
    assert k.batch_stats() == (stats[0] + 2, stats[1] + 2 * B, stats[2])
    gt.fill_(2.0)
    gh = np.full((B, npar), 2.0)
    stats = k.batch_stats()

    def untouched():
        k.synchronize()
        return bool((gt == 2.0).all()) and (gh == 2.0).all() and k.batch_stats() == stats
    bad = boxes.copy()
    bad[1] = np.diag([0.9, 0.77, 0.9])                   # cutoff 0.39 > 0.385: names conformation 1
    for call in (lambda: k.execute_batch_hvp_vjp_device(pt, vt, gt, ut, boxes=bad),
                 lambda: k.execute_batch_hvp_vjp_host(confs, vec, ubar, boxes=bad)):
        with pytest.raises(ChargeFluxError) as ei:
            call()
        assert ei.value.code == _cabi.CF_ERR_INVALID and "conformation 1" in str(ei.value) and untouched()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ptr = lambda t: C.c_void_p(t.data_ptr())
    dev = [k._h, B, ptr(pt), dp(boxes), K, ptr(vt), ptr(ut), ptr(gt)]
    host = [k._h, B, dp(confs), dp(boxes), K, dp(vec), dp(ubar), dp(gh)]
    for fn, args in ((lib.cf_compute_batch_periodic_hvp_vjp, dev), (lib.cf_compute_batch_periodic_hvp_vjp_host, host)):
        for at, value in ((2, None), (3, None), (5, None), (7, None), (1, -1), (4, -1)):
            assert fn(*(args[:at] + [value] + args[at + 1:])) == _cabi.CF_ERR_INVALID
        assert fn(*(args[:1] + [0] + args[2:])) == _cabi.CF_OK   # nconf = 0: a no-op that counts nothing
    assert untouched()
    k.begin(pt[0], boxes[0])                             # between cf_compute_begin and _end
    with pytest.raises(ChargeFluxError) as ei:
        k.execute_batch_hvp_vjp_device(pt, vt, gt, ut, boxes=boxes)
    assert ei.value.code == _cabi.CF_ERR_STATE
    k.end()
    assert untouched()
    system, force, box, confs, boxes, vec, ubar = _inputs("w100")   # several ranks
    k2 = HipCalcCoulForceKernel(rank=0, world_size=2).initialize(system, force)
    with pytest.raises(ChargeFluxError) as ei:
        k2.execute_batch_hvp_vjp_host(confs, vec, ubar, boxes=boxes)
    assert ei.value.code == _cabi.CF_ERR_STATE
