"""GPU tests of cf_compute_batch_esp and cf_compute_batch_esp_vjp (include/chargeflux.h; DESIGN.md
"Batched, electrostatic potential") against tests/esp_reference.py (pinned by test_batch_esp_cpu.py).
Systems: the `_cluster` recipe, B = 3: (1, 0), 3 atoms; (0, 5), no terms; (21, 7), 70 atoms; (100, 21),
321 atoms: across the 256-atom LDS tile and 41 atom tiles of the adjoint.  npts: 1; 77 (a partial
wave); 300 (across a 256-point tile); chunk + 5 (the several-chunk adjoint).  Bars: V and the base rows
a, |d| <= 1e-12 S per entry, S the sum of the magnitudes of the entry's own terms (round-off of an
N-term fp64 sum with a few-ulp rsqrt: below N 4 eps S = 3e-13 S at N = 321; the adjoint's tree sum over
M points grows with log M); whole rows, 1e-9 max |grad| + 1e-9.  Observed on MI355X: DESIGN.md.
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
from tests import esp_reference as er  # noqa: E402
from tests.test_gpu_batch_vjp import _cluster, _conformations, _counts  # noqa: E402

B = 3
CHUNK = _cabi.CF_BATCH_ESP_CHUNK
CASES = [(nw, ni, m) for nw, ni in ((1, 0), (0, 5), (21, 7), (100, 21)) for m in (1, 77, 300)] \
    + [(2, 1, CHUNK + 5), (21, 7, CHUNK + 5)]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _inputs(force, pos, npts, seed):
    confs = _conformations(pos, seed)
    points, closest = ts.probe_points(confs, npts, seed + 500 + npts)
    assert closest >= 0.05
    vbar = np.random.default_rng(seed + 31).normal(size=(B, npts))
    return confs, points, vbar, er.evaluate_batch(force, confs, points, vbar)


@functools.lru_cache(maxsize=None)
def _case(nw, ni, npts):
    """(system, force, conformations, points, cotangent, reference): computed once, shared, read-only."""
    system, force, pos = _cluster(nw, ni)
    return (system, force) + _inputs(force, pos, npts, 177 + nw + ni)


def _fails(code, *calls, text=""):
    for call in calls:
        with pytest.raises(ChargeFluxError) as ei:
            call()
        assert ei.value.code == code and text in str(ei.value)


def _check_vjp(tag, k, confs, points, vbar, ref):
    n = confs.shape[1]
    g = k.execute_batch_esp_vjp_host(confs, points, vbar)["flat"]
    assert np.isfinite(g).all()
    rel = (np.abs(g[:, :n] - ref["a"]) / ref["S_a"]).max()
    err, scale = np.abs(g - ref["grad"]).max(), np.abs(g).max()
    print(f"{tag}: max|a - ref|/S = {rel:.3e}, max|grad - ref| = {err:.3e}, max|grad| = {scale:.3e}")
    assert rel <= 1e-12
    assert err <= 1e-9 * scale + 1e-9
    return g


@pytest.mark.parametrize("nw,ni,npts", CASES)
def test_potentials_and_gradients_match_the_reference(nw, ni, npts):
    system, force, confs, points, vbar, ref = _case(nw, ni, npts)
    k = HipCalcCoulForceKernel().initialize(system, force)
    V, q = k.execute_batch_esp_host(confs, points)
    rel = (np.abs(V - ref["V"]) / ref["S_V"]).max()
    print(f"{nw}+{ni}, M = {npts}: max|V - ref|/S = {rel:.3e}")
    assert np.isfinite(V).all() and rel <= 1e-12
    assert np.array_equal(q, k.execute_batch_host(confs, False, False)[2])   # bitwise cf_compute_batch's
    assert k.param_counts() == _counts(force)
    g = _check_vjp(f"{nw}+{ni}, M = {npts}", k, confs, points, vbar, ref)
    # the identity the closed form rests on: the charge VJP of the batch with q_bar = a
    want = k.execute_batch_vjp_host(confs, charges_bar=np.ascontiguousarray(g[:, :confs.shape[1]]))["flat"]
    assert np.abs(g - want).max() <= 1e-12 * np.abs(g).max()


@pytest.mark.parametrize("nw,ni", [(2, 1), (100, 21)])
def test_bitwise_guarantees(nw, ni):
    system, force, pos = _cluster(nw, ni)
    confs, points, vbar, ref = _inputs(force, pos, 300, 177 + nw + ni)
    stream = torch.cuda.Stream()
    k = HipCalcCoulForceKernel(stream=stream.cuda_stream).initialize(system, force)
    cut = lambda a, s: np.ascontiguousarray(a[s])
    c0, n0, p0 = k.batch_stats()
    V, q = k.execute_batch_esp_host(confs, points)
    g = k.execute_batch_esp_vjp_host(confs, points, vbar)["flat"]
    assert k.batch_stats() == (c0 + 2, n0 + 2 * B, p0 + 2)       # one pass each under the automatic limit
    for b in range(B):                                           # alone (B = 1) = its row of the batch
        s = slice(b, b + 1)
        Vb, qb = k.execute_batch_esp_host(cut(confs, s), cut(points, s))
        assert np.array_equal(Vb[0], V[b]) and np.array_equal(qb[0], q[b])
        assert np.array_equal(k.execute_batch_esp_vjp_host(cut(confs, s), cut(points, s), cut(vbar, s))["flat"][0], g[b])
    rev = slice(None, None, -1)                                  # another place in the batch
    assert np.array_equal(k.execute_batch_esp_host(cut(confs, rev), cut(points, rev))[0][::-1], V)
    assert np.array_equal(k.execute_batch_esp_vjp_host(cut(confs, rev), cut(points, rev), cut(vbar, rev))["flat"][::-1], g)
    p1 = k.batch_stats()[2]
    k.set_batch_limit(1)                                         # one conformation per pass
    assert np.array_equal(k.execute_batch_esp_host(confs, points)[0], V)
    assert np.array_equal(k.execute_batch_esp_vjp_host(confs, points, vbar)["flat"], g)
    assert k.batch_stats()[2] == p1 + 2 * B
    k.set_batch_limit(0)
    few = (slice(None), slice(0, 77))                            # a point does not depend on the others
    assert np.array_equal(k.execute_batch_esp_host(confs, cut(points, few))[0], V[:, :77])
    dev = lambda a: torch.tensor(a, device="cuda:0")             # the device form, over NaN-filled outputs
    nan = lambda a: torch.full(a.shape, float("nan"), dtype=torch.float64, device="cuda:0")
    pt, rt, vt, Vt, qt, gt = dev(confs), dev(points), dev(vbar), nan(V), nan(q), nan(g)
    torch.cuda.synchronize()   # the inputs exist before the side stream reads them
    k.execute_batch_esp_device(pt, rt, Vt, qt)
    k.execute_batch_esp_vjp_device(pt, rt, gt, vt)
    stream.synchronize()
    for got, want in ((Vt, V), (qt, q), (gt, g)):
        assert np.array_equal(got.cpu().numpy(), want)


def test_null_paths_isolation_and_an_update_to_k_zero():
    system, force, pos = _cluster(21, 7, seed=5)
    force = copy.deepcopy(force)
    confs, points, vbar, ref = _inputs(force, pos, 77, 11)
    k = HipCalcCoulForceKernel().initialize(system, force)
    np_ = sum(_counts(force))
    e0, f0 = k.execute_host(confs[0])
    diag = (k.charges(), k.dedq(), k.energy_terms())
    batch = k.execute_batch_host(confs)
    V0, q0 = k.execute_batch_esp_host(confs, points)
    # no cotangent: exact zeros whatever the array held; counted, no pass.  No output: counted
    stats = k.batch_stats()
    assert np.array_equal(k.execute_batch_esp_vjp_host(confs, points)["flat"], np.zeros((B, np_)))
    pt, rt = torch.tensor(confs, device="cuda:0"), torch.tensor(points, device="cuda:0")
    gt = torch.full((B, np_), float("nan"), dtype=torch.float64, device="cuda:0")
    k.execute_batch_esp_vjp_device(pt, rt, gt)
    k.execute_batch_esp_device(pt, rt)
    k.synchronize()
    assert (gt == 0.0).all()
    assert k.batch_stats() == (stats[0] + 3, stats[1] + 3 * B, stats[2])
    # cf_compute's diagnostics and the batch's results are unchanged around the new calls
    for a, b in zip(diag, (k.charges(), k.dedq(), k.energy_terms())):
        assert np.array_equal(a, b)
    e1, f1 = k.execute_host(confs[0])
    assert e1 == e0 and np.array_equal(f1, f0)
    for a, b in zip(batch, k.execute_batch_host(confs)):
        assert np.array_equal(a, b)
    # a parameter update takes effect on the next call; it leaves one term of each kind with k = 0
    for i in range(force.getNumParticles()):
        q, s, e = force.getParticleParameters(i)
        force.setParticleParameters(i, q * 1.05, s, e)
    force._fwater_par = [(k1 * 1.1, k2, kub, b0, ub0) for k1, k2, kub, b0, ub0 in force._fwater_par]
    force._fwater_par[0] = (0.0, 0.0, 0.0) + tuple(force._fwater_par[0][3:])
    force._fbond_par[0], force._fangle_par[0] = (0.0, force._fbond_par[0][1]), (0.0, force._fangle_par[0][1])
    k.copyParametersToContext(force)
    ref = er.evaluate_batch(force, confs, points, vbar)
    V1 = k.execute_batch_esp_host(confs, points)[0]
    assert np.abs(V1 - V0).max() > 1e-3 and (np.abs(V1 - ref["V"]) <= 1e-12 * ref["S_V"]).all()
    _check_vjp("21+7, updated, k = 0", k, confs, points, vbar, ref)


def test_argument_errors():
    lib = _cabi.load_library()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    system, force, pos, box = ts.water_box(100, cutoff=0.6)      # a periodic handle
    kp = HipCalcCoulForceKernel().initialize(system, force)
    one, pts = np.ascontiguousarray(pos[None]), np.ones((1, 4, 3))
    _fails(_cabi.CF_ERR_INVALID, lambda: kp.execute_batch_esp_host(one, pts),
           lambda: kp.execute_batch_esp_vjp_host(one, pts, np.ones((1, 4))), text="non-periodic")
    system, force, confs, points, vbar, ref = _case(0, 5, 77)
    k = HipCalcCoulForceKernel().initialize(system, force)
    n, M = confs.shape[1], 77
    pt, rt, vt = (torch.tensor(a, device="cuda:0") for a in (confs, points, vbar))
    two = lambda *shape: torch.full(shape, 2.0, dtype=torch.float64, device="cuda:0")
    gt, Vt, qt = two(B, n), two(B, M), two(B, n)
    stats = k.batch_stats()
    esp, vjp = lib.cf_compute_batch_esp, lib.cf_compute_batch_esp_vjp
    # nconf = 0 and npts = 0: OK, nothing written (the charges included), nothing counted
    for nconf, npts in ((0, M), (B, 0)):
        assert esp(k._h, nconf, ptr(pt), npts, ptr(rt), ptr(Vt), ptr(qt)) == _cabi.CF_OK
        assert vjp(k._h, nconf, ptr(pt), npts, ptr(rt), ptr(vt), ptr(gt)) == _cabi.CF_OK
    assert k.execute_batch_esp_host(np.zeros((0, n, 3)), np.zeros((0, M, 3)))[0].shape == (0, M)
    assert k.execute_batch_esp_vjp_host(confs, np.zeros((B, 0, 3)))["flat"].shape == (B, n)
    # negative counts, null positions, points, grad
    for bad in ((-1, ptr(pt), M, ptr(rt)), (B, ptr(pt), -1, ptr(rt)), (B, None, M, ptr(rt)), (B, ptr(pt), M, None)):
        assert esp(k._h, *bad, ptr(Vt), None) == _cabi.CF_ERR_INVALID
        assert vjp(k._h, *bad, ptr(vt), ptr(gt)) == _cabi.CF_ERR_INVALID
    assert vjp(k._h, B, ptr(pt), M, ptr(rt), ptr(vt), None) == _cabi.CF_ERR_INVALID
    assert lib.cf_compute_batch_esp_host(k._h, B, None, M, None, None, None) == _cabi.CF_ERR_INVALID
    assert lib.cf_compute_batch_esp_vjp_host(k._h, B, None, M, None, None, None) == _cabi.CF_ERR_INVALID
    k.synchronize()
    assert (gt == 2.0).all() and (Vt == 2.0).all() and (qt == 2.0).all() and k.batch_stats() == stats
    k.begin(pt[0])                                               # between cf_compute_begin and _end
    _fails(_cabi.CF_ERR_STATE, lambda: k.execute_batch_esp_device(pt, rt, Vt), lambda: k.execute_batch_esp_vjp_device(pt, rt, gt, vt))
    k.end()
    k.synchronize()
    k2 = HipCalcCoulForceKernel(rank=0, world_size=2).initialize(system, force)   # several ranks
    _fails(_cabi.CF_ERR_STATE, lambda: k2.execute_batch_esp_host(confs, points), lambda: k2.execute_batch_esp_vjp_host(confs, points, vbar))


def test_torch_layer_matches_the_host_vjp():
    from openmmcoul.fitting import BatchedChargeFlux
    system, force, pos = _cluster(21, 7)
    force = copy.deepcopy(force)
    k = HipCalcCoulForceKernel().initialize(system, force)
    confs, points, target, _ = _inputs(force, pos, 77, 41)
    model = BatchedChargeFlux(k, force)
    pt, rt, tt = (torch.tensor(a, device="cuda:0") for a in (confs, points, target))
    params = model.parameters(device="cuda:0")
    V = model.esp(*params, pt, rt)
    host = k.execute_batch_esp_host(confs, points)[0]
    assert V.shape == (B, 77) and np.array_equal(V.detach().cpu().numpy(), host)
    ((V - tt) ** 2).sum().backward()
    want = k.execute_batch_esp_vjp_host(confs, points, np.ascontiguousarray(2.0 * (host - target)))
    for p, name in zip(params, ("charges", "bonds", "angles", "waters")):
        w = want[name].sum(axis=0)
        assert np.abs(p.grad.cpu().numpy().reshape(w.shape) - w).max() <= 1e-12 * max(1.0, np.abs(w).max()), name
    for bad in ((pt.clone().requires_grad_(True), rt), (pt, rt.clone().requires_grad_(True))):
        with pytest.raises(ValueError):
            model.esp(*params, *bad)
