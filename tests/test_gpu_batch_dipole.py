"""GPU tests of the dipoles and atomic polar tensors of the non-periodic batch
(cf_compute_batch_dipole, cf_compute_batch_dipole_vjp; include/chargeflux.h; DESIGN.md "Batched,
dipoles and polar tensors"): against the numpy restatement of the formulas
(tests/dipole_reference.py, itself pinned to the oracle by tests/test_batch_dipole_cpu.py), the
bitwise guarantees, isolation from the single-evaluation state, parameter updates, the argument errors
and the torch layer (BatchedChargeFlux.dipoles).

Systems: the `_cluster` recipe of test_gpu_batch_vjp.py, B = 3 conformations: (1 water, 0 ions);
(0, 5), no terms; (2, 1); (21, 7), 70 atoms, across one wave; (100, 21), 321 atoms, across a 256 tile
with a tail, its bond-and-angle waters giving an oxygen 7 chain-rule entries (across the gather's
batch of 4).

Bars.  Forward: max |d| <= 1e-12 max(1, max |ref|) for mu and P (sums of at most 321 terms of size
<= ~2: round-off below 1e-13); the charges bitwise those of cf_compute_batch.  VJP: the project's bar
max |grad - ref| <= 1e-9 max |grad| + 1e-9 against the reference gradient, per system and cotangent
set, over every parameter of every system (the reference is a closed form, so (100, 21) needs no
sampling: every sample is included).  Observed on MI355X (printed by the tests): see DESIGN.md.
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
from tests import dipole_reference as dr  # noqa: E402
from tests.test_gpu_batch_vjp import _cluster, _conformations, _counts  # noqa: E402

B = 3
REL, ABS = 1e-9, 1e-9
SIZES = [(1, 0), (0, 5), (2, 1), (21, 7), (100, 21)]
SETS = ("mu", "P", "both")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _cotangents(n, seed):
    rng = np.random.default_rng(seed)
    mb, pb = rng.normal(size=(B, 3)), rng.normal(size=(B, n, 3, 3))
    return {"mu": (mb, None), "P": (None, pb), "both": (mb, pb)}


@functools.lru_cache(maxsize=None)
def _case(nw, ni):
    """(system, force, conformations, cotangents, reference {set: q, mu, P, grad}): the reference runs
    once per system and is shared, read-only."""
    system, force, pos = _cluster(nw, ni)
    confs = _conformations(pos, 177 + nw + ni)
    cots = _cotangents(pos.shape[0], 31 + nw + ni)
    ref = {s: dr.evaluate_batch(force, confs, *cots[s]) for s in SETS}
    return system, force, confs, cots, ref


def _kernel(nw, ni, **kw):
    system, force = _case(nw, ni)[:2]
    return HipCalcCoulForceKernel(**kw).initialize(system, force)


def _check_gradient(tag, g, ref):
    assert np.isfinite(g).all()
    err = np.abs(g - ref).max()
    scale = np.abs(g).max()
    print(f"{tag}: max|grad - ref| = {err:.3e}, max|grad| = {scale:.3e}")
    assert err <= REL * scale + ABS, (tag, err, scale)


# 1 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nw,ni", SIZES)
def test_forward_matches_the_reference(nw, ni):
    system, force, confs, cots, ref = _case(nw, ni)
    r = ref["both"]
    k = _kernel(nw, ni)
    mu, apt, q = k.execute_batch_dipole_host(confs)
    for name, got, want in (("mu", mu, r["mu"]), ("P", apt, r["P"])):
        err, scale = np.abs(got - want).max(), np.abs(want).max()
        print(f"{nw}+{ni}: max|{name} - ref| = {err:.3e}, max|{name}| = {scale:.3e}")
        assert err <= 1e-12 * max(1.0, scale)
    assert np.array_equal(q, k.execute_batch_host(confs, False, False)[2])   # bitwise cf_compute_batch's
    assert np.abs(q - r["q"]).max() <= 1e-13
    if (nw, ni) == (0, 5):   # no terms: P_b = q_b I exactly
        assert np.array_equal(apt, q[:, :, None, None] * np.eye(3))


# 2 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nw,ni", SIZES)
def test_vjp_matches_the_reference_gradient(nw, ni):
    system, force, confs, cots, ref = _case(nw, ni)
    k = _kernel(nw, ni)
    assert k.param_counts() == _counts(force)
    for s in SETS:
        g = k.execute_batch_dipole_vjp_host(confs, *cots[s])["flat"]
        _check_gradient(f"{nw}+{ni} [{s}]", g, ref[s]["grad"])


def test_a_term_with_k_zero():
    system, force, pos = _cluster(21, 7)
    force = copy.deepcopy(force)
    force._fbond_par[0] = (0.0, force._fbond_par[0][1])
    force._fangle_par[0] = (0.0, force._fangle_par[0][1])
    k1, k2, kub, b0, ub0 = force._fwater_par[0]
    force._fwater_par[0] = (0.0, 0.0, 0.0, b0, ub0)
    confs = _conformations(pos, 19)
    mb, pb = _cotangents(pos.shape[0], 23)["both"]
    k = HipCalcCoulForceKernel().initialize(system, force)
    r = dr.evaluate_batch(force, confs, mb, pb)
    g = k.execute_batch_dipole_vjp_host(confs, mb, pb)["flat"]
    _check_gradient("21+7, k = 0", g, r["grad"])
    mu, apt, q = k.execute_batch_dipole_host(confs)
    assert np.abs(apt - r["P"]).max() <= 1e-12 * max(1.0, np.abs(r["P"]).max())
    assert np.abs(mu - r["mu"]).max() <= 1e-12 * max(1.0, np.abs(r["mu"]).max())


@pytest.mark.parametrize("nw,ni", [(21, 7), (100, 21)])
def test_linearity_and_null_cotangents(nw, ni):
    system, force, confs, cots, ref = _case(nw, ni)
    k = _kernel(nw, ni)
    g = {s: k.execute_batch_dipole_vjp_host(confs, *cots[s])["flat"] for s in SETS}
    d = np.abs(g["both"] - (g["mu"] + g["P"])).max()
    print(f"{nw}+{ni}: linearity max|d| = {d:.3e}, max|grad| = {np.abs(g['both']).max():.3e}")
    assert d <= 1e-12 * np.abs(g["both"]).max()
    mb, pb = cots["both"]
    g2 = k.execute_batch_dipole_vjp_host(confs, 2.0 * mb, np.ascontiguousarray(-0.5 * pb))["flat"]
    assert np.abs(g2 - (2.0 * g["mu"] - 0.5 * g["P"])).max() <= 1e-12 * np.abs(g["both"]).max()
    # no cotangent: exact zeros whatever the array held; the call is counted, no pass
    np_ = sum(_counts(force))
    stats = k.batch_stats()
    out = k.execute_batch_dipole_vjp_host(confs)
    assert np.array_equal(out["flat"], np.zeros((B, np_)))
    assert k.batch_stats() == (stats[0] + 1, stats[1] + B, stats[2])
    pt = torch.tensor(confs, device="cuda:0")
    gt = torch.full((B, np_), 7.0, dtype=torch.float64, device="cuda:0")
    k.execute_batch_dipole_vjp_device(pt, gt)
    k.synchronize()
    assert (gt == 0.0).all()
    assert k.batch_stats() == (stats[0] + 2, stats[1] + 2 * B, stats[2])
    # the forward call with no output: counted, nothing launched
    k.execute_batch_dipole_device(pt)
    k.synchronize()
    assert k.batch_stats() == (stats[0] + 3, stats[1] + 3 * B, stats[2])
    assert out["waters"].shape == (B, force.getNumFluxWaters(), 5)


# 3 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nw,ni", [(2, 1), (100, 21)])
def test_bitwise_guarantees(nw, ni):
    system, force, confs, cots, ref = _case(nw, ni)
    k = _kernel(nw, ni)
    mb, pb = cots["both"]
    c0, n0, p0 = k.batch_stats()
    fwd = k.execute_batch_dipole_host(confs)
    assert k.batch_stats() == (c0 + 1, n0 + B, p0 + 1)          # one pass under the automatic limit
    g = k.execute_batch_dipole_vjp_host(confs, mb, pb)["flat"]
    assert k.batch_stats() == (c0 + 2, n0 + 2 * B, p0 + 2)
    for b in range(B):                                          # alone (B = 1) = its row of the batch
        one = np.ascontiguousarray(confs[b:b + 1])
        for got, want in zip(k.execute_batch_dipole_host(one), fwd):
            assert np.array_equal(got[0], want[b])
        gb = k.execute_batch_dipole_vjp_host(one, np.ascontiguousarray(mb[b:b + 1]), np.ascontiguousarray(pb[b:b + 1]))
        assert np.array_equal(gb["flat"][0], g[b])
    rev = np.ascontiguousarray(confs[::-1])                     # another place in the batch
    for got, want in zip(k.execute_batch_dipole_host(rev), fwd):
        assert np.array_equal(got[::-1], want)
    gr = k.execute_batch_dipole_vjp_host(rev, np.ascontiguousarray(mb[::-1]), np.ascontiguousarray(pb[::-1]))["flat"]
    assert np.array_equal(gr[::-1], g)
    p1 = k.batch_stats()[2]
    k.set_batch_limit(1)                                        # one conformation per pass
    for got, want in zip(k.execute_batch_dipole_host(confs), fwd):
        assert np.array_equal(got, want)
    assert np.array_equal(k.execute_batch_dipole_vjp_host(confs, mb, pb)["flat"], g)
    assert k.batch_stats()[2] == p1 + 2 * B
    k.set_batch_limit(0)


def test_device_form_overwrites_and_equals_the_host_form():
    stream = torch.cuda.Stream()
    system, force, confs, cots, ref = _case(100, 21)
    k = _kernel(100, 21, stream=stream.cuda_stream)
    mb, pb = cots["both"]
    mu, apt, q = k.execute_batch_dipole_host(confs)
    g = k.execute_batch_dipole_vjp_host(confs, mb, pb)["flat"]
    dev = lambda a: torch.tensor(a, device="cuda:0")
    garbage = lambda a: torch.full(a.shape, float("nan"), dtype=torch.float64, device="cuda:0")
    pt, mt, at, qt, gt = dev(confs), garbage(mu), garbage(apt), garbage(q), garbage(g)
    mbt, pbt = dev(mb), dev(pb)
    torch.cuda.synchronize()   # the inputs exist before the side stream reads them
    k.execute_batch_dipole_device(pt, mt, at, qt)
    k.execute_batch_dipole_vjp_device(pt, gt, mbt, pbt)
    stream.synchronize()
    for got, want in ((mt, mu), (at, apt), (qt, q), (gt, g)):
        assert np.array_equal(got.cpu().numpy(), want)
    # each output alone
    mt2, at2 = garbage(mu), garbage(apt)
    k.execute_batch_dipole_device(pt, dipoles=mt2)
    k.execute_batch_dipole_device(pt, apts=at2)
    stream.synchronize()
    assert np.array_equal(mt2.cpu().numpy(), mu) and np.array_equal(at2.cpu().numpy(), apt)


# 4 ------------------------------------------------------------------------------------------
def test_isolation_from_the_single_evaluation_state():
    system, force, confs, cots, ref = _case(21, 7)
    k = _kernel(21, 7)
    e0, f0 = k.execute_host(confs[0])
    diag = (k.charges(), k.dedq(), k.energy_terms())
    k.execute_batch_dipole_host(np.ascontiguousarray(confs[1:]))
    k.execute_batch_dipole_vjp_host(np.ascontiguousarray(confs[1:]), cots["both"][0][1:].copy(), cots["both"][1][1:].copy())
    for a, b in zip(diag, (k.charges(), k.dedq(), k.energy_terms())):
        assert np.array_equal(a, b)
    e1, f1 = k.execute_host(confs[0])
    assert e1 == e0 and np.array_equal(f1, f0)
    # the forward batch shares the workspace: neither disturbs the other
    e, f, q = k.execute_batch_host(confs)
    fwd = k.execute_batch_dipole_host(confs)
    e2, f2, q2 = k.execute_batch_host(confs)
    assert np.array_equal(e, e2) and np.array_equal(f, f2) and np.array_equal(q, q2)
    for a, b in zip(fwd, k.execute_batch_dipole_host(confs)):
        assert np.array_equal(a, b)


def test_parameter_update_takes_effect_on_the_next_call():
    system, force, pos = _cluster(21, 7, seed=5)
    force = copy.deepcopy(force)
    confs = _conformations(pos, 11)
    mb, pb = _cotangents(pos.shape[0], 13)["both"]
    k = HipCalcCoulForceKernel().initialize(system, force)
    mu0, apt0, q0 = k.execute_batch_dipole_host(confs)
    for i in range(force.getNumParticles()):
        q, s, e = force.getParticleParameters(i)
        force.setParticleParameters(i, q * 1.05, s, e)
    for w in range(force.getNumFluxWaters()):
        k1, k2, kub, b0, ub0 = force._fwater_par[w]
        force._fwater_par[w] = (k1 * 1.1, k2, kub, b0, ub0)
    k.copyParametersToContext(force)
    mu1, apt1, q1 = k.execute_batch_dipole_host(confs)
    assert np.abs(apt1 - apt0).max() > 1e-3 and np.abs(mu1 - mu0).max() > 1e-3   # the update took effect
    r = dr.evaluate_batch(force, confs, mb, pb)
    assert np.abs(apt1 - r["P"]).max() <= 1e-12 * max(1.0, np.abs(r["P"]).max())
    assert np.abs(mu1 - r["mu"]).max() <= 1e-12 * max(1.0, np.abs(r["mu"]).max())
    _check_gradient("21+7, updated", k.execute_batch_dipole_vjp_host(confs, mb, pb)["flat"], r["grad"])


# 5 ------------------------------------------------------------------------------------------
def test_argument_errors():
    lib = _cabi.load_library()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    # periodic handle
    system, force, pos, box = ts.water_box(100, cutoff=0.6)
    kp = HipCalcCoulForceKernel().initialize(system, force)
    for call in (kp.execute_batch_dipole_host, lambda p: kp.execute_batch_dipole_vjp_host(p, dipole_bar=np.ones((1, 3)))):
        with pytest.raises(ChargeFluxError) as ei:
            call(np.ascontiguousarray(pos[None]))
        assert ei.value.code == _cabi.CF_ERR_INVALID and "non-periodic" in str(ei.value)
    # nconf = 0: OK, nothing written, nothing counted
    system, force, confs, cots, ref = _case(0, 5)
    k = _kernel(0, 5)
    n = confs.shape[1]
    pt = torch.tensor(confs, device="cuda:0")
    mb = torch.ones((B, 3), dtype=torch.float64, device="cuda:0")
    gt = torch.full((B, n), 2.0, dtype=torch.float64, device="cuda:0")
    mt = torch.full((B, 3), 2.0, dtype=torch.float64, device="cuda:0")
    stats = k.batch_stats()
    assert lib.cf_compute_batch_dipole(k._h, 0, ptr(pt), ptr(mt), None, None) == _cabi.CF_OK
    assert lib.cf_compute_batch_dipole_vjp(k._h, 0, ptr(pt), ptr(mb), None, ptr(gt)) == _cabi.CF_OK
    k.synchronize()
    assert k.batch_stats() == stats
    assert (gt == 2.0).all() and (mt == 2.0).all()
    assert k.execute_batch_dipole_vjp_host(np.zeros((0, n, 3)))["flat"].shape == (0, n)
    assert k.execute_batch_dipole_host(np.zeros((0, n, 3)))[1].shape == (0, n, 3, 3)
    # negative nconf, null positions, null grad
    assert lib.cf_compute_batch_dipole(k._h, -1, ptr(pt), ptr(mt), None, None) == _cabi.CF_ERR_INVALID
    assert lib.cf_compute_batch_dipole(k._h, B, None, ptr(mt), None, None) == _cabi.CF_ERR_INVALID
    assert lib.cf_compute_batch_dipole_host(k._h, B, None, None, None, None) == _cabi.CF_ERR_INVALID
    assert lib.cf_compute_batch_dipole_vjp(k._h, -1, ptr(pt), ptr(mb), None, ptr(gt)) == _cabi.CF_ERR_INVALID
    assert lib.cf_compute_batch_dipole_vjp(k._h, B, None, ptr(mb), None, ptr(gt)) == _cabi.CF_ERR_INVALID
    assert lib.cf_compute_batch_dipole_vjp(k._h, B, ptr(pt), ptr(mb), None, None) == _cabi.CF_ERR_INVALID
    assert lib.cf_compute_batch_dipole_vjp_host(k._h, B, None, None, None, None) == _cabi.CF_ERR_INVALID
    k.synchronize()
    assert (gt == 2.0).all() and (mt == 2.0).all() and k.batch_stats() == stats
    # between cf_compute_begin and _end
    k.begin(pt[0])
    for call in (lambda: k.execute_batch_dipole_device(pt, mt), lambda: k.execute_batch_dipole_vjp_device(pt, gt, mb)):
        with pytest.raises(ChargeFluxError) as ei:
            call()
        assert ei.value.code == _cabi.CF_ERR_STATE
    k.end()
    k.synchronize()
    # several ranks
    system, force, confs2 = _case(21, 7)[:3]
    k2 = HipCalcCoulForceKernel(rank=0, world_size=2).initialize(system, force)
    for call in (lambda: k2.execute_batch_dipole_host(confs2),
                 lambda: k2.execute_batch_dipole_vjp_host(confs2, dipole_bar=np.ones((B, 3)))):
        with pytest.raises(ChargeFluxError) as ei:
            call()
        assert ei.value.code == _cabi.CF_ERR_STATE


# 6 ------------------------------------------------------------------------------------------
def test_torch_layer_matches_the_host_vjp():
    from openmmcoul.fitting import BatchedChargeFlux
    system, force, pos = _cluster(21, 7)
    force = copy.deepcopy(force)
    k = HipCalcCoulForceKernel().initialize(system, force)
    confs = _conformations(pos, 41)
    n = pos.shape[0]
    rng = np.random.default_rng(43)
    target, weight = rng.normal(size=(B, 3)), rng.normal(size=(B, n, 3, 3))
    model = BatchedChargeFlux(k, force)
    pt = torch.tensor(confs, device="cuda:0")
    t, w = torch.tensor(target, device="cuda:0"), torch.tensor(weight, device="cuda:0")
    names = ("charges", "bonds", "angles", "waters")

    def close(params, host):
        for p, name in zip(params, names):
            want = host[name].sum(axis=0)
            got = p.grad.cpu().numpy().reshape(want.shape)
            assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), name

    params = model.parameters(device="cuda:0")
    dipoles, apts = model.dipoles(*params, pt)
    assert dipoles.shape == (B, 3) and apts.shape == (B, n, 3, 3)
    mu, apt, _ = k.execute_batch_dipole_host(confs)
    assert np.array_equal(dipoles.detach().cpu().numpy(), mu) and np.array_equal(apts.detach().cpu().numpy(), apt)
    loss = ((dipoles - t) ** 2).sum() + (apts * w).sum()
    loss.backward()
    close(params, k.execute_batch_dipole_vjp_host(confs, np.ascontiguousarray(2.0 * (mu - target)), weight))
    # only the dipoles used: the APT cotangent arrives as None (a NULL cotangent)
    seen = []
    vjp = k.execute_batch_dipole_vjp_device
    k.execute_batch_dipole_vjp_device = lambda p, g, mb=None, pb=None: (seen.append((mb, pb)), vjp(p, g, mb, pb))[1]
    params = model.parameters(device="cuda:0")
    dipoles, apts = model.dipoles(*params, pt)
    ((dipoles - t) ** 2).sum().backward()
    assert len(seen) == 1 and seen[0][0] is not None and seen[0][1] is None
    close(params, k.execute_batch_dipole_vjp_host(confs, np.ascontiguousarray(2.0 * (mu - target))))
    with pytest.raises(ValueError):
        model.dipoles(*params, pt.clone().requires_grad_(True))
