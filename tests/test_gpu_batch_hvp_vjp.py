"""GPU tests of cf_compute_batch_hvp_vjp (include/chargeflux.h; DESIGN.md "Batched, Hessian-vector
parameter gradients") against central differences of the complex-step products
(tests/hvp_vjp_reference.py, checked by tests/test_batch_hvp_vjp_cpu.py).  `_cluster` systems, B = 2,
seeded N(0, 1) directions and cotangents; the reference rows are computed once per system.
Bar: max|grad - ref| <= 1e-9 max|ref| + 1e-9 per parameter group; observed on MI355X: see DESIGN.md.
"""
import copy
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from openmmcoul import ChargeFluxError, HipCalcCoulForceKernel, _cabi  # noqa: E402
from openmmcoul import testsystems as ts  # noqa: E402
from openmmcoul.fitting import BatchedChargeFlux  # noqa: E402
from tests import hvp_reference as hr  # noqa: E402
from tests import hvp_vjp_reference as hvr  # noqa: E402
from tests.test_gpu_batch_vjp import _cluster, _conformations, _counts  # noqa: E402

B, KC = 2, 4   # KC: the directions a block of the pair kernel carries
REL, ABS = 1e-9, 1e-9


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _inputs(force, pos, seed, nvec=KC + 1):
    confs = np.ascontiguousarray(_conformations(pos, seed)[:B])
    vecs, ubar = np.random.default_rng(seed + 1).normal(size=(2, B, nvec) + pos.shape)
    return confs, vecs, ubar


def _reference_rows(force, confs, vecs, ubar):
    ref = hr.Reference(force)
    return np.stack([hvr.grad_rows(ref, confs[b], vecs[b], ubar[b]) for b in range(len(confs))])   # (B,K,P)


@functools.lru_cache(maxsize=None)
def _case(nw, ni):
    """(system, force, conformations, directions, cotangents, reference rows (B,K,P)); (100, 21) is
    compared along parameter directions only and has no rows."""
    system, force, pos = _cluster(nw, ni)
    confs, vecs, ubar = _inputs(force, pos, 277 + nw + ni)
    return system, force, confs, vecs, ubar, None if nw == 100 else _reference_rows(force, confs, vecs, ubar)


def _kernel(nw, ni):
    system, force = _case(nw, ni)[:2]
    return HipCalcCoulForceKernel().initialize(system, force)


_check = functools.partial(hvr.check_groups, rel=REL, ab=ABS)


def _cut(a, nvec):
    return np.ascontiguousarray(a[:, :nvec])


@pytest.mark.parametrize("nvec", [1, KC, KC + 1])
@pytest.mark.parametrize("nw,ni", [(1, 0), (0, 5), (2, 1), (21, 7)])
def test_matches_the_reference_per_parameter(nw, ni, nvec):
    system, force, confs, vecs, ubar, rows = _case(nw, ni)
    got = _kernel(nw, ni).execute_batch_hvp_vjp_host(confs, _cut(vecs, nvec), _cut(ubar, nvec))["flat"]
    _check(f"{nw}+{ni} K={nvec}", got, rows[:, :nvec].sum(axis=1), _counts(force))
    if (nw, ni) == (1, 0):   # every pair excluded: no energy at all
        assert np.array_equal(got, np.zeros_like(got))


def test_matches_the_reference_along_parameter_directions():
    system, force, confs, vecs, ubar, _ = _case(100, 21)   # N = 321: several i-tiles, a j-tile with a tail
    confs, vecs, ubar = confs[:1], _cut(vecs[:1], 2), _cut(ubar[:1], 2)
    ref = hr.Reference(force)
    dirs = hvr.seeded_directions(ref, 91, 3)
    want = np.array([hvr.directional(ref, confs[0], vecs[0], ubar[0], d).sum() for d in dirs])
    got = _kernel(100, 21).execute_batch_hvp_vjp_host(confs, vecs, ubar)["flat"][0] @ dirs.T
    _check("100+21 base and k-type", got[:3], want[:3], (3,))
    _check("100+21 ref-type", got[3:], want[3:], (3,))


def test_symmetry_and_aliasing():
    system, force, confs, vecs, ubar, _ = _case(21, 7)
    k = _kernel(21, 7)
    g = k.execute_batch_hvp_vjp_host(confs, vecs, ubar)["flat"]
    swapped = k.execute_batch_hvp_vjp_host(confs, ubar, vecs)["flat"]
    print(f"21+7: max|g(u,v) - g(v,u)| = {np.abs(g - swapped).max():.3e}, max|g| = {np.abs(g).max():.3e}")
    assert np.abs(g - swapped).max() <= 1e-12 * np.abs(g).max()
    assert np.array_equal(k.execute_batch_hvp_vjp_host(confs, vecs, vecs)["flat"],
                          k.execute_batch_hvp_vjp_host(confs, vecs, vecs.copy())["flat"])


@pytest.mark.parametrize("nw,ni", [(2, 1), (100, 21)])
def test_bitwise_guarantees(nw, ni):
    system, force, confs, vecs, ubar, _ = _case(nw, ni)
    k = _kernel(nw, ni)
    run = lambda sel: k.execute_batch_hvp_vjp_host(*(np.ascontiguousarray(a[sel]) for a in (confs, vecs, ubar)))["flat"]
    c0, n0, p0 = k.batch_stats()
    g = run(slice(None))
    assert k.batch_stats() == (c0 + 1, n0 + B, p0 + 1)          # as execute_batch_hvp_host: one pass
    assert np.array_equal(run(slice(None)), g)
    for b in range(B):                                          # alone = its row of the batch
        assert np.array_equal(run(slice(b, b + 1))[0], g[b])
    assert np.array_equal(run(slice(None, None, -1))[::-1], g)  # any position of the batch
    p1 = k.batch_stats()[2]
    k.set_batch_limit(1)
    assert np.array_equal(run(slice(None)), g) and k.batch_stats()[2] == p1 + B
    k.set_batch_limit(0)
    gt = torch.empty(g.shape, dtype=torch.float64, device="cuda:0")
    k.execute_batch_hvp_vjp_device(*(torch.tensor(a, device="cuda:0") for a in (confs, vecs)), gt,
                                   torch.tensor(ubar, device="cuda:0"))
    k.synchronize()
    assert np.array_equal(gt.cpu().numpy(), g)


def test_directions_split_over_passes():
    system, force, confs, vecs, ubar, _ = _case(2, 1)
    k = _kernel(2, 1)
    conf, real = confs[:1], 3
    pad = 65536
    v = np.zeros((1, pad + real) + confs.shape[1:])
    u = np.random.default_rng(7).normal(size=v.shape)
    v[:, pad:], u[:, pad:] = vecs[:1, :real], ubar[:1, :real]
    p0 = k.batch_stats()[2]
    g = k.execute_batch_hvp_vjp_host(conf, v, u)["flat"]
    assert k.batch_stats()[2] > p0 + 1
    # every term carries a factor from v: the zero rows add exact zeros to the running sums
    assert np.array_equal(g, k.execute_batch_hvp_vjp_host(conf, _cut(vecs[:1], real), _cut(ubar[:1], real))["flat"])


def test_k_zero_and_parameter_updates():
    system, force, pos = _cluster(2, 1)
    force = copy.deepcopy(force)
    force._fbond_par[0] = (0.0, force._fbond_par[0][1])
    force._fangle_par[0] = (0.0, force._fangle_par[0][1])
    force._fwater_par[0] = (0.0, 0.0, 0.0) + tuple(force._fwater_par[0][3:])
    confs, vecs, ubar = _inputs(force, pos, 19, nvec=2)
    k = HipCalcCoulForceKernel().initialize(system, force)
    g0 = k.execute_batch_hvp_vjp_host(confs, vecs, ubar)["flat"]
    _check("2+1, k = 0", g0, _reference_rows(force, confs, vecs, ubar).sum(axis=1), _counts(force))
    for i in range(force.getNumParticles()):
        q, s, e = force.getParticleParameters(i)
        force.setParticleParameters(i, q * 1.05, s, e)
    force._fwater_par[0] = (-1.1, 0.2, 0.5) + tuple(force._fwater_par[0][3:])
    k.copyParametersToContext(force)
    g1 = k.execute_batch_hvp_vjp_host(confs, vecs, ubar)["flat"]
    assert np.abs(g1 - g0).max() > 1e-3 * np.abs(g0).max()      # the update took effect
    _check("2+1, updated", g1, _reference_rows(force, confs, vecs, ubar).sum(axis=1), _counts(force))


def test_torch_layer():
    system, force, confs, vecs, ubar, _ = _case(2, 1)
    force = copy.deepcopy(force)
    k = HipCalcCoulForceKernel().initialize(system, force)
    model = BatchedChargeFlux(k, force)
    params = model.parameters()
    pt, vt, wt = (torch.tensor(a, device="cuda:0") for a in (confs, vecs, ubar))
    out = model.hvp(*params, pt, vt)
    assert np.array_equal(out.detach().cpu().numpy(), k.execute_batch_hvp_host(confs, vecs))
    (wt * out).sum().backward()
    want = k.execute_batch_hvp_vjp_host(confs, vecs, ubar)
    for p, name in zip(params, ("charges", "bonds", "angles", "waters")):
        assert np.array_equal(p.grad.numpy(), torch.tensor(want[name]).sum(dim=0).numpy()), name


def test_argument_errors_and_overwriting():
    lib = _cabi.load_library()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    system, force, pos, box = ts.water_box(100, cutoff=0.6)
    kp = HipCalcCoulForceKernel().initialize(system, force)
    with pytest.raises(ChargeFluxError) as ei:
        kp.execute_batch_hvp_vjp_host(np.ascontiguousarray(pos[None]), np.ones((1, 1) + pos.shape))
    assert ei.value.code == _cabi.CF_ERR_INVALID and "non-periodic" in str(ei.value)
    system, force, confs, vecs, ubar, _ = _case(0, 5)
    k = _kernel(0, 5)
    nvec, n = vecs.shape[1], confs.shape[1]
    pt, vt, ut = (torch.tensor(a, device="cuda:0") for a in (confs, vecs, ubar))
    gt = torch.full((B, sum(k.param_counts())), float("nan"), dtype=torch.float64, device="cuda:0")
    k.execute_batch_hvp_vjp_device(pt, vt, gt, ut)              # grad is overwritten, not added to
    k.synchronize()
    assert np.array_equal(gt.cpu().numpy(), k.execute_batch_hvp_vjp_host(confs, vecs, ubar)["flat"])
    stats = k.batch_stats()
    for zero in (k.execute_batch_hvp_vjp_host(confs, vecs)["flat"],                      # out_bar = None
                 k.execute_batch_hvp_vjp_host(confs, *np.zeros((2, B, 0, n, 3)))["flat"]):   # the empty sum
        assert zero.shape == gt.shape and not zero.any()
    assert k.batch_stats() == (stats[0] + 2, stats[1] + 2 * B, stats[2])
    gt.fill_(2.0)
    stats = k.batch_stats()
    call = lambda nc, p, nv, v, u, g: lib.cf_compute_batch_hvp_vjp(k._h, nc, p, nv, v, u, g)
    assert call(0, ptr(pt), nvec, ptr(vt), ptr(ut), ptr(gt)) == _cabi.CF_OK           # nconf = 0 counts nothing
    assert call(-1, ptr(pt), nvec, ptr(vt), ptr(ut), ptr(gt)) == _cabi.CF_ERR_INVALID
    assert call(B, ptr(pt), -1, ptr(vt), ptr(ut), ptr(gt)) == _cabi.CF_ERR_INVALID
    assert call(B, None, nvec, ptr(vt), ptr(ut), ptr(gt)) == _cabi.CF_ERR_INVALID
    assert call(B, ptr(pt), nvec, None, ptr(ut), ptr(gt)) == _cabi.CF_ERR_INVALID
    assert call(B, ptr(pt), nvec, ptr(vt), ptr(ut), None) == _cabi.CF_ERR_INVALID
    assert lib.cf_compute_batch_hvp_vjp_host(k._h, B, None, nvec, None, None, None) == _cabi.CF_ERR_INVALID
    k.synchronize()
    assert (gt == 2.0).all() and k.batch_stats() == stats
    k.begin(pt[0])
    with pytest.raises(ChargeFluxError) as ei:
        k.execute_batch_hvp_vjp_device(pt, vt, gt, ut)
    assert ei.value.code == _cabi.CF_ERR_STATE
    k.end()
    k.synchronize()
    system, force, pos = _cluster(64, 64)
    k2 = HipCalcCoulForceKernel(rank=0, world_size=2).initialize(system, force)
    with pytest.raises(ChargeFluxError) as ei:
        k2.execute_batch_hvp_vjp_host(np.ascontiguousarray(pos[None]), np.ones((1, 1) + pos.shape))
    assert ei.value.code == _cabi.CF_ERR_STATE
