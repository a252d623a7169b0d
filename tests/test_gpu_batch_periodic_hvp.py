"""GPU tests of the Hessian-vector products of the periodic batch (cf_compute_batch_periodic_hvp,
include/chargeflux.h; DESIGN.md "Batched, periodic, Hessian-vector products").  Systems, boxes and
conformations: the recipes of test_gpu_batch_periodic_vjp.py (B = 3 boxes scaled per axis, in
conformation 1 every fifth atom moved by a whole box vector), K = 6 seeded N(0, 1) directions: with 4
directions per chunk a full chunk and a tail.  The yardstick is the complex step through
tests/pbc_hvp_reference.py (guarded on the CPU by test_batch_periodic_hvp_cpu.py).
Condition on the inputs (asserted, not a tolerance): no non-excluded minimum-image pair within 1e-9 nm
of the cutoff and no minimum-image component within 1e-9 nm of a face.
Bar of test 1: max|out - ref| <= 1e-9 max|ref| + 1e-9 over the whole (B,K,N,3) array, the bar of the
non-periodic products and of the periodic parameter gradients.  Observed on MI355X: see DESIGN.md.
"""
import copy
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import Oracle  # noqa: E402
from openmmcoul import ChargeFluxError, HipCalcCoulForceKernel, _cabi  # noqa: E402
from openmmcoul import testsystems as ts  # noqa: E402
from tests import pbc_hvp_reference as pr  # noqa: E402
from tests.test_gpu_batch_periodic_vjp import (B, SYSTEMS, _assert_clear_of_cutoff, _conformations,  # noqa: E402
                                               _min_image, _system)

K = 6
REL, ABS = 1e-9, 1e-9


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """(system, force, default box, conformations, boxes, directions (B,K,N,3)); the input condition."""
    system, force, pos, box = _system(name)
    confs, boxes = _conformations(name, pos, box, 400 + SYSTEMS.index(name))
    for x, bb in zip(confs, boxes):
        _assert_clear_of_cutoff(force, x, bb)
        d = _min_image(x[None, :, :] - x[:, None, :], bb)[~np.eye(len(x), dtype=bool)]
        assert np.abs(np.abs(d) - 0.5 * np.diag(bb)).min() > 1e-9
    vec = np.random.default_rng(700 + SYSTEMS.index(name)).normal(size=(B, K) + pos.shape)
    return system, force, box, confs, boxes, vec


def _reference(force, box, confs, boxes, vec):
    ref = pr.Reference(force, *Oracle(force, box).ewald())
    return np.stack([np.stack([ref.hv(x, bb, v) for v in vs]) for x, bb, vs in zip(confs, boxes, vec)])


@functools.lru_cache(maxsize=None)
def _expected(name):
    system, force, box, confs, boxes, vec = _inputs(name)
    return _reference(force, box, confs, boxes, vec)


def _kernel(name, **kw):
    system, force = _inputs(name)[:2]
    return HipCalcCoulForceKernel(**kw).initialize(system, force)


def _check(tag, out, ref):
    err, scale = np.abs(out - ref).max(), np.abs(ref).max()
    print(f"{tag}: max|out - ref| = {err:.3e}, max|ref| = {scale:.3e}, ratio = {err / scale:.3e}")
    assert np.isfinite(out).all() and err <= REL * scale + ABS, (tag, err, scale)


@pytest.mark.parametrize("name", SYSTEMS)
def test_matches_the_complex_step_reference(name):
    system, force, box, confs, boxes, vec = _inputs(name)
    k = _kernel(name)
    out = k.execute_batch_hvp_host(confs, vec, boxes=boxes)
    _check(name, out, _expected(name))
    one = k.execute_batch_hvp_host(confs, np.ascontiguousarray(vec[:, K - 1:]), boxes=boxes)   # K = 1: the last
    _check(name + ", K = 1", one, _expected(name)[:, K - 1:])
    assert k.device_errors() == 0


def test_full_hessian_is_symmetric_with_translations_as_null_vectors():
    system, force, box, confs, boxes, vec = _inputs("w22")
    h = _kernel("w22").hessians_host(confs, symmetrize=False, boxes=boxes)
    n = confs.shape[1]
    for b in range(B):
        hmax, asym = np.abs(h[b]).max(), np.abs(h[b] - h[b].T).max()
        null = max(np.abs(h[b].reshape(3 * n, n, 3)[:, :, a].sum(axis=1)).max() for a in range(3))
        print(f"w22 conformation {b}: max|H - H^T| = {asym:.3e}, max|H t| = {null:.3e}, max|H| = {hmax:.3e}")
        assert asym <= 1e-12 * hmax and null <= 1e-9 * hmax


@pytest.mark.parametrize("name", ["ions", "w100", "tric"])
def test_bitwise_guarantees(name):
    stream = torch.cuda.Stream()
    system, force, box, confs, boxes, vec = _inputs(name)
    k = _kernel(name, stream=stream.cuda_stream)
    run = lambda x, v, bb: k.execute_batch_hvp_host(np.ascontiguousarray(x), np.ascontiguousarray(v),
                                                    boxes=np.ascontiguousarray(bb))
    stats = k.batch_stats()
    g = run(confs, vec, boxes)
    assert k.batch_stats() == (stats[0] + 1, stats[1] + B, stats[2] + 1)   # one pass under the automatic limit
    assert np.array_equal(run(confs, vec, boxes), g)
    for b in range(B):                                   # alone = its row of the batch
        assert np.array_equal(run(confs[b:b + 1], vec[b:b + 1], boxes[b:b + 1])[0], g[b])
    for s in (0, K - 1):                                 # K = 1 = its slot of K = 6
        assert np.array_equal(run(confs, vec[:, s:s + 1], boxes), g[:, s:s + 1])
    perm = [3, 5, 0, 4, 1, 2]                            # every direction in another chunk slot
    assert np.array_equal(run(confs, vec[:, perm], boxes), g[:, perm])
    assert np.array_equal(run(confs[::-1], vec[::-1], boxes[::-1])[::-1], g)
    p1 = k.batch_stats()[2]
    k.set_batch_limit(2)
    assert np.array_equal(run(confs, vec, boxes), g) and k.batch_stats()[2] == p1 + 2   # 2 + 1 conformations
    k.set_batch_limit(0)
    pt, vt = torch.tensor(confs, device="cuda:0"), torch.tensor(vec, device="cuda:0")
    ot = torch.full(vec.shape, float("nan"), dtype=torch.float64, device="cuda:0")      # out is overwritten
    torch.cuda.synchronize()   # the inputs exist before the side stream reads them
    bx = boxes.copy()
    k.execute_batch_hvp_device(pt, vt, ot, boxes=bx)
    bx[:] = np.nan             # the boxes are the caller's again as soon as the call returns
    stream.synchronize()
    assert np.array_equal(ot.cpu().numpy(), g) and k.device_errors() == 0


def test_terms_with_k_zero_and_a_parameter_update():
    system, force, box, confs, boxes, vec = _inputs("w22")
    force = copy.deepcopy(force)
    k = HipCalcCoulForceKernel().initialize(system, force)
    g0 = k.execute_batch_hvp_host(confs, vec, boxes=boxes)
    force._fbond_par[0] = (0.0, force._fbond_par[0][1])
    force._fangle_par[0] = (0.0, force._fangle_par[0][1])
    force._fwater_par[0] = (0.0, 0.0, 0.0) + tuple(force._fwater_par[0][3:])
    for i in range(force.getNumParticles()):
        q, s, e = force.getParticleParameters(i)
        force.setParticleParameters(i, q * 1.05, s, e)
    k.copyParametersToContext(force)
    g1 = k.execute_batch_hvp_host(confs, vec, boxes=boxes)
    assert np.abs(g1 - g0).max() > 1e-3 * np.abs(g0).max()   # the update took effect
    _check("w22, k = 0, updated", g1[1:2], _reference(force, box, confs[1:2], boxes[1:2], vec[1:2]))


def test_isolation_from_the_single_evaluation_state_and_the_other_periodic_batches():
    system, force, box, confs, boxes, vec = _inputs("w100")
    k = _kernel("w100", kspace_algo=HipCalcCoulForceKernel.KSPACE_GRID)
    fb = np.random.default_rng(3).normal(size=confs.shape)
    e0, f0 = k.execute_host(confs[0], boxes[0])
    fwd = k.execute_batch_host(confs, boxes=boxes)
    vjp = k.execute_batch_vjp_host(confs, forces_bar=fb, boxes=boxes)["flat"]
    diag, stats = (k.charges(), k.dedq(), k.energy_terms()), k.batch_stats()
    k.execute_batch_hvp_host(confs, vec, boxes=boxes)
    assert k.batch_stats() == (stats[0] + 1, stats[1] + B, stats[2] + 1)
    assert all(np.array_equal(a, b) for a, b in zip(diag, (k.charges(), k.dedq(), k.energy_terms())))
    e1, f1 = k.execute_host(confs[0], boxes[0])
    assert e1 == e0 and np.array_equal(f1, f0)
    assert all(np.array_equal(a, b) for a, b in zip(fwd, k.execute_batch_host(confs, boxes=boxes)))
    assert np.array_equal(k.execute_batch_vjp_host(confs, forces_bar=fb, boxes=boxes)["flat"], vjp)
    assert k.device_errors() == 0


def test_argument_errors():
    lib = _cabi.load_library()
    system, force, cpos, _ = ts.cluster_c1()             # a non-periodic handle with boxes
    kn = HipCalcCoulForceKernel().initialize(system, force)
    with pytest.raises(ChargeFluxError) as ei:
        kn.execute_batch_hvp_host(np.ascontiguousarray(cpos[None]), np.ones((1, 1) + cpos.shape), boxes=np.eye(3) * 3.0)
    assert ei.value.code == _cabi.CF_ERR_INVALID and "periodic" in str(ei.value)
    system, force, box, confs, boxes, vec = _inputs("w22")
    k = _kernel("w22")
    g = k.execute_batch_hvp_host(confs, vec, boxes=boxes)
    stats = k.batch_stats()
    pt, vt = torch.tensor(confs, device="cuda:0"), torch.tensor(vec, device="cuda:0")
    ot = torch.full(vec.shape, 2.0, dtype=torch.float64, device="cuda:0")
    oh = np.full(vec.shape, 2.0)

    def untouched():
        k.synchronize()
        return bool((ot == 2.0).all()) and (oh == 2.0).all() and k.batch_stats() == stats
    bad = boxes.copy()
    bad[1] = np.diag([0.9, 0.77, 0.9])                   # cutoff 0.39 > 0.385: names conformation 1
    for call in (lambda: k.execute_batch_hvp_device(pt, vt, ot, boxes=bad),
                 lambda: k.execute_batch_hvp_host(confs, vec, boxes=bad)):
        with pytest.raises(ChargeFluxError) as ei:
            call()
        assert ei.value.code == _cabi.CF_ERR_INVALID and "conformation 1" in str(ei.value) and untouched()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ptr = lambda t: C.c_void_p(t.data_ptr())
    dev = [k._h, B, ptr(pt), dp(boxes), K, ptr(vt), ptr(ot)]
    host = [k._h, B, dp(confs), dp(boxes), K, dp(vec), dp(oh)]
    for fn, args in ((lib.cf_compute_batch_periodic_hvp, dev), (lib.cf_compute_batch_periodic_hvp_host, host)):
        for at, value in ((2, None), (3, None), (5, None), (6, None), (1, -1), (4, -1)):
            assert fn(*(args[:at] + [value] + args[at + 1:])) == _cabi.CF_ERR_INVALID
        for at in (1, 4):                                # nconf = 0 or nvec = 0: a no-op that counts nothing
            assert fn(*(args[:at] + [0] + args[at + 1:])) == _cabi.CF_OK
    assert untouched()
    k.begin(pt[0], boxes[0])                             # between cf_compute_begin and _end
    with pytest.raises(ChargeFluxError) as ei:
        k.execute_batch_hvp_device(pt, vt, ot, boxes=boxes)
    assert ei.value.code == _cabi.CF_ERR_STATE
    k.end()
    assert untouched()
    assert np.array_equal(k.execute_batch_hvp_host(confs, vec, boxes=boxes), g)   # still works, the same bits
    system, force, box, confs, boxes, vec = _inputs("w100")   # several ranks
    k2 = HipCalcCoulForceKernel(rank=0, world_size=2).initialize(system, force)
    with pytest.raises(ChargeFluxError) as ei:
        k2.execute_batch_hvp_host(confs, vec, boxes=boxes)
    assert ei.value.code == _cabi.CF_ERR_STATE
