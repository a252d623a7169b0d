"""GPU tests of the Hessian-vector products of the non-periodic batch (cf_compute_batch_hvp,
include/chargeflux.h; DESIGN.md "Batched, Hessian-vector products"): against the complex-step
reference (tests/hvp_reference.py, itself checked on the CPU by tests/test_batch_hvp_cpu.py), the
full Hessian's symmetry and null vectors, linearity, the bitwise guarantees, a term with k = 0,
isolation from the single-evaluation state, parameter updates and the argument errors.

Systems: the `_cluster` recipe of test_gpu_batch_vjp.py, B = 3 conformations, K = 3 seeded N(0, 1)
directions per conformation (K = 1: the third of them).

Bar (every comparison with the reference): max|out - ref| <= 1e-9 max|ref| + 1e-9, the maxima over
the whole (B,K,N,3) array.  Observed on MI355X (printed by the tests): see DESIGN.md.
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
from tests import hvp_reference as hr  # noqa: E402
from tests.test_gpu_batch_vjp import _cluster, _conformations  # noqa: E402

B, K = 3, 3
REL, ABS = 1e-9, 1e-9
# (waters, ions): every pair excluded; no terms (a pure pair Hessian); small; across one wave; across
# the 64-atom i-tiles and a 256-entry j-tile with a tail
SIZES = [(1, 0), (0, 5), (2, 1), (21, 7), (100, 21)]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _reference_hv(force, confs, vecs):
    ref = hr.Reference(force)
    return np.stack([np.stack([ref.hv(confs[b], vecs[b, k]) for k in range(vecs.shape[1])])
                     for b in range(len(confs))])


@functools.lru_cache(maxsize=None)
def _case(nw, ni):
    """(system, force, conformations (B,N,3), directions (B,K,N,3), reference H v (B,K,N,3)): the
    reference runs once per system and is shared, read-only."""
    system, force, pos = _cluster(nw, ni)
    confs = _conformations(pos, 177 + nw + ni)
    vecs = np.random.default_rng(61 + nw + ni).normal(size=(B, K) + pos.shape)
    return system, force, confs, vecs, _reference_hv(force, confs, vecs)


def _kernel(nw, ni, **kw):
    system, force = _case(nw, ni)[:2]
    return HipCalcCoulForceKernel(**kw).initialize(system, force)


def _check(tag, out, ref):
    assert out.shape == ref.shape and np.isfinite(out).all()
    err, scale = np.abs(out - ref).max(), np.abs(ref).max()
    ratio = f"{err / scale:.3e}" if scale > 0 else "-"
    print(f"{tag}: max|Hv - ref| = {err:.3e}, max|ref| = {scale:.3e}, ratio = {ratio}")
    assert err <= REL * scale + ABS, (tag, err, scale)


def _last(vecs):
    return np.ascontiguousarray(vecs[:, K - 1:K])


# 1 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nw,ni", SIZES)
def test_matches_the_complex_step_reference(nw, ni):
    system, force, confs, vecs, ref = _case(nw, ni)
    k = _kernel(nw, ni)
    _check(f"{nw}+{ni} K=3", k.execute_batch_hvp_host(confs, vecs), ref)
    _check(f"{nw}+{ni} K=1", k.execute_batch_hvp_host(confs, _last(vecs)), ref[:, K - 1:K])
    if (nw, ni) == (1, 0):   # every pair excluded: no energy at all
        assert np.array_equal(k.execute_batch_hvp_host(confs, vecs), np.zeros_like(vecs))


# 2 ------------------------------------------------------------------------------------------
def test_full_hessian():
    system, force, confs, vecs, _ = _case(2, 1)
    k = _kernel(2, 1)
    n3 = 3 * confs.shape[1]
    raw = k.hessians_host(confs, symmetrize=False)
    assert raw.shape == (B, n3, n3)
    ref = hr.Reference(force)
    for b in range(B):
        hmax = np.abs(raw[b]).max()
        asym = np.abs(raw[b] - raw[b].T).max()
        print(f"2+1 conformation {b}: max|H - H^T| = {asym:.3e}, max|H| = {hmax:.3e}")
        assert asym <= 1e-12 * hmax
        for axis in range(3):
            t = np.zeros((confs.shape[1], 3))
            t[:, axis] = 1.0
            null = np.abs(raw[b] @ t.ravel()).max()
            print(f"    translation {axis}: max|H t| = {null:.3e}")
            assert null <= 1e-9 * hmax
        _check(f"2+1 conformation {b}, full Hessian", raw[b].T, ref.hessian(confs[b]))   # row k = H e_k
    sym = k.hessians_host(confs)
    assert np.array_equal(sym, 0.5 * (raw + raw.transpose(0, 2, 1)))
    assert np.array_equal(sym, sym.transpose(0, 2, 1))


# 3 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nw,ni", [(21, 7), (100, 21)])
def test_linearity_and_the_zero_vector(nw, ni):
    system, force, confs, vecs, _ = _case(nw, ni)
    k = _kernel(nw, ni)
    u, v = vecs[:, 0:1], vecs[:, 1:2]
    combo = np.ascontiguousarray(2.0 * u - 0.5 * v)
    h = k.execute_batch_hvp_host(confs, vecs)
    hc = k.execute_batch_hvp_host(confs, combo)
    d = np.abs(hc - (2.0 * h[:, 0:1] - 0.5 * h[:, 1:2])).max()
    print(f"{nw}+{ni}: linearity max|d| = {d:.3e}, max|Hv| = {np.abs(hc).max():.3e}")
    assert d <= 1e-12 * np.abs(hc).max()
    zero = np.zeros_like(vecs)
    assert np.array_equal(k.execute_batch_hvp_host(confs, zero), zero)


# 4 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nw,ni", [(2, 1), (100, 21)])
def test_bitwise_guarantees(nw, ni):
    system, force, confs, vecs, _ = _case(nw, ni)
    k = _kernel(nw, ni)
    c0, n0, p0 = k.batch_stats()
    h = k.execute_batch_hvp_host(confs, vecs)
    assert k.batch_stats() == (c0 + 1, n0 + B, p0 + 1)          # one pass under the automatic limit
    assert np.array_equal(k.execute_batch_hvp_host(confs, vecs), h)
    for b in range(B):                                          # alone (B = 1) = its rows of the batch
        hb = k.execute_batch_hvp_host(np.ascontiguousarray(confs[b:b + 1]), np.ascontiguousarray(vecs[b:b + 1]))
        assert np.array_equal(hb[0], h[b])
    h1 = k.execute_batch_hvp_host(confs, _last(vecs))           # K = 1 = slot 2 of K = 3
    assert np.array_equal(h1[:, 0], h[:, K - 1])
    hr_ = k.execute_batch_hvp_host(np.ascontiguousarray(confs[::-1]), np.ascontiguousarray(vecs[::-1, ::-1]))
    assert np.array_equal(hr_[::-1, ::-1], h)                   # any position of the batch
    p1 = k.batch_stats()[2]
    k.set_batch_limit(2)
    h2 = k.execute_batch_hvp_host(confs, vecs)
    assert k.batch_stats()[2] == p1 + 2                         # 2 + 1 conformations
    assert np.array_equal(h2, h)
    k.set_batch_limit(0)
    # the device form
    pt, vt = torch.tensor(confs, device="cuda:0"), torch.tensor(vecs, device="cuda:0")
    ot = k.execute_batch_hvp_device(pt, vt)
    k.synchronize()
    assert np.array_equal(ot.cpu().numpy(), h)


# 5 ------------------------------------------------------------------------------------------
def test_a_term_of_each_kind_with_k_zero():
    system, force, pos = _cluster(21, 7)
    force = copy.deepcopy(force)
    force._fbond_par[0] = (0.0, force._fbond_par[0][1])
    force._fangle_par[0] = (0.0, force._fangle_par[0][1])
    k1, k2, kub, b0, ub0 = force._fwater_par[0]
    force._fwater_par[0] = (0.0, 0.0, 0.0, b0, ub0)
    confs = _conformations(pos, 19)
    vecs = np.random.default_rng(23).normal(size=(B, K) + pos.shape)
    k = HipCalcCoulForceKernel().initialize(system, force)
    _check("21+7, k = 0", k.execute_batch_hvp_host(confs, vecs), _reference_hv(force, confs, vecs))


# 6 ------------------------------------------------------------------------------------------
def test_isolation_from_the_single_evaluation_state():
    system, force, confs, vecs, ref = _case(21, 7)
    k = _kernel(21, 7)
    e0, f0 = k.execute_host(confs[0])
    q0 = k.charges()
    stats = k.batch_stats()
    h = k.execute_batch_hvp_host(confs, vecs)
    assert k.batch_stats() == (stats[0] + 1, stats[1] + B, stats[2] + 1)
    assert np.array_equal(k.charges(), q0)                      # still that cf_compute's charges
    e1, f1 = k.execute_host(confs[0])
    assert e1 == e0 and np.array_equal(f1, f0)
    # the forward batch and the products share a workspace: neither disturbs the other
    e, f, q = k.execute_batch_host(confs)
    assert np.array_equal(k.execute_batch_hvp_host(confs, vecs), h)
    e2, f2, q2 = k.execute_batch_host(confs)
    assert np.array_equal(e, e2) and np.array_equal(f, f2) and np.array_equal(q, q2)


def test_parameter_update_reaches_the_products():
    system, force, pos = _cluster(21, 7, seed=5)
    force = copy.deepcopy(force)
    confs = _conformations(pos, 11)
    vecs = np.random.default_rng(13).normal(size=(B, K) + pos.shape)
    k = HipCalcCoulForceKernel().initialize(system, force)
    h0 = k.execute_batch_hvp_host(confs, vecs)
    for i in range(force.getNumParticles()):
        q, s, e = force.getParticleParameters(i)
        force.setParticleParameters(i, q * 1.05, s, e)
    for w in range(force.getNumFluxWaters()):
        k1, k2, kub, b0, ub0 = force._fwater_par[w]
        force._fwater_par[w] = (k1 * 1.1, k2, kub, b0, ub0)
    k.copyParametersToContext(force)
    h1 = k.execute_batch_hvp_host(confs, vecs)
    assert np.abs(h1 - h0).max() > 1e-3 * np.abs(h0).max()      # the update took effect
    _check("21+7, updated", h1, _reference_hv(force, confs, vecs))


# 7 ------------------------------------------------------------------------------------------
def test_argument_errors_and_overwriting():
    lib = _cabi.load_library()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    # periodic handle
    system, force, pos, box = ts.water_box(100, cutoff=0.6)
    kp = HipCalcCoulForceKernel().initialize(system, force)
    with pytest.raises(ChargeFluxError) as ei:
        kp.execute_batch_hvp_host(np.ascontiguousarray(pos[None]), np.ones((1, 1) + pos.shape))
    assert ei.value.code == _cabi.CF_ERR_INVALID and "non-periodic" in str(ei.value)
    # out is overwritten, not added to
    system, force, confs, vecs, ref = _case(0, 5)
    k = _kernel(0, 5)
    n = confs.shape[1]
    pt, vt = torch.tensor(confs, device="cuda:0"), torch.tensor(vecs, device="cuda:0")
    ot = torch.full((B, K, n, 3), float("nan"), dtype=torch.float64, device="cuda:0")
    assert k.execute_batch_hvp_device(pt, vt, out=ot) is ot
    k.synchronize()
    assert np.array_equal(ot.cpu().numpy(), k.execute_batch_hvp_host(confs, vecs))
    # nconf = 0 and nvec = 0: OK, nothing written, nothing counted
    ot.fill_(2.0)
    stats = k.batch_stats()
    assert lib.cf_compute_batch_hvp(k._h, 0, ptr(pt), K, ptr(vt), ptr(ot)) == _cabi.CF_OK
    assert lib.cf_compute_batch_hvp(k._h, B, ptr(pt), 0, ptr(vt), ptr(ot)) == _cabi.CF_OK
    k.synchronize()
    assert k.batch_stats() == stats and (ot == 2.0).all()
    assert k.execute_batch_hvp_host(np.zeros((0, n, 3)), np.zeros((0, K, n, 3))).shape == (0, K, n, 3)
    assert k.execute_batch_hvp_host(confs, np.zeros((B, 0, n, 3))).shape == (B, 0, n, 3)
    assert k.batch_stats() == stats
    # negative counts, null pointers
    assert lib.cf_compute_batch_hvp(k._h, -1, ptr(pt), K, ptr(vt), ptr(ot)) == _cabi.CF_ERR_INVALID
    assert lib.cf_compute_batch_hvp(k._h, B, ptr(pt), -1, ptr(vt), ptr(ot)) == _cabi.CF_ERR_INVALID
    assert lib.cf_compute_batch_hvp(k._h, B, None, K, ptr(vt), ptr(ot)) == _cabi.CF_ERR_INVALID
    assert lib.cf_compute_batch_hvp(k._h, B, ptr(pt), K, None, ptr(ot)) == _cabi.CF_ERR_INVALID
    assert lib.cf_compute_batch_hvp(k._h, B, ptr(pt), K, ptr(vt), None) == _cabi.CF_ERR_INVALID
    assert lib.cf_compute_batch_hvp_host(k._h, B, None, K, None, None) == _cabi.CF_ERR_INVALID
    k.synchronize()
    assert (ot == 2.0).all() and k.batch_stats() == stats
    # between cf_compute_begin and _end
    k.begin(pt[0])
    with pytest.raises(ChargeFluxError) as ei:
        k.execute_batch_hvp_device(pt, vt, out=ot)
    assert ei.value.code == _cabi.CF_ERR_STATE
    k.end()
    k.synchronize()
    # several ranks
    system, force, pos = _cluster(64, 64)
    k2 = HipCalcCoulForceKernel(rank=0, world_size=2).initialize(system, force)
    with pytest.raises(ChargeFluxError) as ei:
        k2.execute_batch_hvp_host(np.ascontiguousarray(pos[None]), np.ones((1, 1) + pos.shape))
    assert ei.value.code == _cabi.CF_ERR_STATE
