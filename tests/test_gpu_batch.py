"""GPU tests of the batched evaluation (cf_compute_batch, include/chargeflux.h):
B conformations of a non-periodic system in one call, against the oracle and against cf_compute
one conformation at a time, plus the bitwise guarantees (independence of the batch, of B and of
the chunking), accumulation, isolation from the single-evaluation state, parameter updates, the
device form and the argument errors.

Systems follow C1's recipe (testsystems.cluster_c1): water centres on a cubic lattice of spacing
0.325 nm at offset 0.25, ion centres on the same lattice at offset 0.75, +-0.02 nm lattice jitter,
waters alternating FluxWater / bond+angle, ions +-1 e, sigma 0.3 nm, eps 0.5 kJ/mol.

Tolerances are the fp64 bars of test_gpu_parity.py:
  forces   max |dF| <= 1e-8 kJ/mol/nm,  energy |dE| <= 1e-9 |E| + 1e-8 kJ/mol,  charges <= 1e-12 e
"""
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

F_TOL = 1e-8
Q_TOL = 1e-12
B = 7
SHIFT = np.array([0.4, -0.2, 0.1])
# (waters, ions): fewer atoms than a wave with every pair excluded; no flux terms and no
# exclusions; across one wave, not a multiple of 64; across a 256 tile with a tail; C1 itself
SIZES = [(1, 0), (0, 5), (21, 7), (100, 21), (64, 64)]
FLAGS = [(True, True), (True, False), (False, True)]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _e_tol(e):
    return 1e-9 * abs(e) + 1e-8


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


@functools.lru_cache(maxsize=None)
def _case(nw, ni):
    """(system, force, conformations (B,N,3), {(fl, en): [oracle result per conformation]}): the
    oracle runs once per system and is shared, read-only, by every test."""
    system, force, pos = _cluster(nw, ni)
    confs = _conformations(pos, 77 + nw + ni)
    o = Oracle(force)
    refs = {fe: [o.execute(confs[b], None, *fe) for b in range(B)] for fe in FLAGS}
    for r in refs[(True, True)]:
        assert np.isfinite(r["forces"]).all() and np.isfinite(r["energy"])
    return system, force, confs, refs


def _kernel(nw, ni, **kw):
    system, force, confs, refs = _case(nw, ni)
    return HipCalcCoulForceKernel(**kw).initialize(system, force), confs, refs


def _report(tag, df, de, dq):
    print(f"{tag}: max|dF| = {df:.3e} kJ/mol/nm, max|dE| = {de:.3e} kJ/mol, max|dq| = {dq:.3e} e")


# 1 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nw,ni", SIZES)
def test_batch_matches_oracle_per_conformation(nw, ni):
    k, confs, refs = _kernel(nw, ni)
    n = confs.shape[1]
    for fl, en in FLAGS:
        pre = np.full((B, n, 3), 0.5)
        e, f, q = k.execute_batch_host(confs, fl, en, forces=pre.copy())
        ref = refs[(fl, en)]
        df = max(np.abs(f[b] - 0.5 - ref[b]["forces"]).max() for b in range(B)) if fl else 0.0
        de = max(abs(e[b] - ref[b]["energy"]) for b in range(B))
        dq = max(np.abs(q[b] - ref[b]["charges"]).max() for b in range(B))
        _report(f"{nw}+{ni} F={fl} E={en}", df, de, dq)
        for b in range(B):
            if fl:
                assert np.abs(f[b] - 0.5 - ref[b]["forces"]).max() <= F_TOL
            assert abs(e[b] - ref[b]["energy"]) <= _e_tol(ref[b]["energy"]), (b, e[b], ref[b]["energy"])
            assert np.abs(q[b] - ref[b]["charges"]).max() <= Q_TOL
        if not fl:
            assert np.array_equal(f, pre)     # untouched, bit for bit
        if not en:
            assert np.array_equal(e, np.zeros(B))


# 2 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nw,ni", SIZES)
def test_batch_matches_cf_compute_one_at_a_time(nw, ni):
    k, confs, _ = _kernel(nw, ni)
    e, f, q = k.execute_batch_host(confs)
    for b in range(B):
        e1, f1 = k.execute_host(confs[b])
        q1 = k.charges()
        assert np.abs(f[b] - f1).max() <= F_TOL
        assert abs(e[b] - e1) <= _e_tol(e1)
        assert np.abs(q[b] - q1).max() <= Q_TOL


# 3 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nw,ni", SIZES)
def test_independence_and_determinism_bitwise(nw, ni):
    k, confs, _ = _kernel(nw, ni)
    c0, _, p0 = k.batch_stats()
    e, f, q = k.execute_batch_host(confs)
    assert k.batch_stats() == (c0 + 1, B, p0 + 1)          # one pass under the automatic limit
    e2, f2, q2 = k.execute_batch_host(confs)
    assert np.array_equal(e, e2) and np.array_equal(f, f2) and np.array_equal(q, q2)
    for b in range(B):                                     # alone (B = 1) = its slice of the batch
        eb, fb, qb = k.execute_batch_host(np.ascontiguousarray(confs[b:b + 1]))
        assert np.array_equal(eb[0], e[b]) and np.array_equal(fb[0], f[b]) and np.array_equal(qb[0], q[b])
    # a different batch around it: reversed order
    er, fr, qr = k.execute_batch_host(np.ascontiguousarray(confs[::-1]))
    assert np.array_equal(er[::-1], e) and np.array_equal(fr[::-1], f) and np.array_equal(qr[::-1], q)
    p1 = k.batch_stats()[2]
    k.set_batch_limit(3)
    e3, f3, q3 = k.execute_batch_host(confs)
    assert k.batch_stats()[2] == p1 + 3                    # 3 + 3 + 1 conformations
    assert np.array_equal(e, e3) and np.array_equal(f, f3) and np.array_equal(q, q3)
    k.set_batch_limit(0)
    p2 = k.batch_stats()[2]
    e4, f4, q4 = k.execute_batch_host(confs)
    assert k.batch_stats()[2] == p2 + 1
    assert np.array_equal(e, e4) and np.array_equal(f, f4) and np.array_equal(q, q4)


# 4 ------------------------------------------------------------------------------------------
def test_accumulation_and_optional_outputs():
    k, confs, refs = _kernel(21, 7)
    n = confs.shape[1]
    e, f, q = k.execute_batch_host(confs)
    # host form: added to a pre-filled buffer; charges optional
    pre = np.random.default_rng(1).normal(size=(B, n, 3))
    e1, f1, q1 = k.execute_batch_host(confs, forces=pre.copy(), return_charges=False)
    assert q1 is None and np.array_equal(e1, e)
    assert np.abs(f1 - (pre + f)).max() <= 1e-12 * np.abs(f).max()
    # device form: forces += on the device, energies and charges overwritten
    pt = torch.tensor(confs, device="cuda:0")
    ft = torch.tensor(pre, device="cuda:0")
    et = torch.full((B,), 123.0, dtype=torch.float64, device="cuda:0")
    qt = torch.full((B, n), -7.0, dtype=torch.float64, device="cuda:0")
    k.execute_batch_device(pt, True, True, ft, et, qt)
    k.synchronize()
    assert np.array_equal(et.cpu().numpy(), e) and np.array_equal(qt.cpu().numpy(), q)
    assert np.array_equal(ft.cpu().numpy(), pre + f)
    # each output may be None
    et.fill_(123.0); qt.fill_(-7.0); ft.zero_()
    k.execute_batch_device(pt, True, True, None, et, qt)
    k.synchronize()
    assert np.array_equal(et.cpu().numpy(), e) and np.array_equal(qt.cpu().numpy(), q)
    et.fill_(123.0); qt.fill_(-7.0)
    k.execute_batch_device(pt, True, True, ft, None, qt)
    k.synchronize()
    assert np.array_equal(ft.cpu().numpy(), f) and np.array_equal(qt.cpu().numpy(), q)
    assert np.array_equal(et.cpu().numpy(), np.full(B, 123.0))
    ft.zero_(); qt.fill_(-7.0)
    k.execute_batch_device(pt, True, True, ft, et, None)
    k.synchronize()
    assert np.array_equal(ft.cpu().numpy(), f) and np.array_equal(et.cpu().numpy(), e)
    assert np.array_equal(qt.cpu().numpy(), np.full((B, n), -7.0))
    # charges alone
    k.execute_batch_device(pt, False, False, None, None, qt)
    k.synchronize()
    assert np.array_equal(qt.cpu().numpy(), q)


# 5 ------------------------------------------------------------------------------------------
def test_isolation_from_the_single_evaluation_state():
    k, confs, refs = _kernel(64, 64)
    e0, f0 = k.execute_host(confs[0])
    diag = (k.charges(), k.dedq(), k.energy_terms(), k.neighbor_stats())
    e, f, q = k.execute_batch_host(confs[1:])
    after = (k.charges(), k.dedq(), k.energy_terms(), k.neighbor_stats())
    for a, b in zip(diag[:3], after[:3]):
        assert np.array_equal(a, b)
    assert diag[3] == after[3]
    e1, f1 = k.execute_host(confs[0])
    assert e1 == e0 and np.array_equal(f1, f0)
    # graph mode on the handle: single evaluations are captured / replayed, batches stay eager
    k.set_graph(True)
    for _ in range(2):
        eg, fg = k.execute_host(confs[0])
        assert eg == e0 and np.array_equal(fg, f0)
    gs = k.graph_stats()
    e2, f2, q2 = k.execute_batch_host(confs[1:])
    assert k.graph_stats() == gs
    assert np.array_equal(e2, e) and np.array_equal(f2, f) and np.array_equal(q2, q)
    ref = refs[(True, True)]
    for b in range(1, B):
        assert np.abs(f2[b - 1] - ref[b]["forces"]).max() <= F_TOL
        assert abs(e2[b - 1] - ref[b]["energy"]) <= _e_tol(ref[b]["energy"])
    eg, fg = k.execute_host(confs[0])
    assert eg == e0 and np.array_equal(fg, f0)


# 6 ------------------------------------------------------------------------------------------
def test_parameter_update_reaches_the_batch_path():
    system, force, pos = _cluster(21, 7, seed=5)
    confs = _conformations(pos, 11)
    k = HipCalcCoulForceKernel().initialize(system, force)
    e0, f0, q0 = k.execute_batch_host(confs)
    for i in range(force.getNumParticles()):
        q, s, e = force.getParticleParameters(i)
        force.setParticleParameters(i, q * 1.05, s, e)
    for w in range(force.getNumFluxWaters()):
        k1, k2, kub, b0, ub0 = force._fwater_par[w]
        force._fwater_par[w] = (k1 * 1.1, k2, kub, b0, ub0)
    k.copyParametersToContext(force)
    e, f, q = k.execute_batch_host(confs)
    assert np.abs(e - e0).min() > 1e-3 * np.abs(e0).max()   # the update took effect
    o = Oracle(force)
    for b in range(B):
        ref = o.execute(confs[b], None)
        assert np.abs(f[b] - ref["forces"]).max() <= F_TOL
        assert abs(e[b] - ref["energy"]) <= _e_tol(ref["energy"])
        assert np.abs(q[b] - ref["charges"]).max() <= Q_TOL


# 7 ------------------------------------------------------------------------------------------
def test_device_form_on_a_side_stream_equals_host_form():
    stream = torch.cuda.Stream()
    k, confs, _ = _kernel(100, 21, stream=stream.cuda_stream)
    n = confs.shape[1]
    e, f, q = k.execute_batch_host(confs)
    pt = torch.tensor(confs, device="cuda:0")
    ft = torch.zeros((B, n, 3), dtype=torch.float64, device="cuda:0")
    et = torch.zeros(B, dtype=torch.float64, device="cuda:0")
    qt = torch.zeros((B, n), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()   # the inputs exist before the side stream reads them
    k.execute_batch_device(pt, True, True, ft, et, qt)
    stream.synchronize()
    assert np.array_equal(et.cpu().numpy(), e)
    assert np.array_equal(ft.cpu().numpy(), f)
    assert np.array_equal(qt.cpu().numpy(), q)


# 8 ------------------------------------------------------------------------------------------
def test_argument_errors():
    lib = _cabi.load_library()
    # periodic handle
    system, force, pos, box = ts.water_box(100, cutoff=0.6)
    kp = HipCalcCoulForceKernel().initialize(system, force)
    with pytest.raises(ChargeFluxError) as ei:
        kp.execute_batch_host(np.ascontiguousarray(pos[None]))
    assert ei.value.code == _cabi.CF_ERR_INVALID and "non-periodic" in str(ei.value)
    # nconf = 0: OK, nothing written, nothing counted
    k, confs, _ = _kernel(0, 5)
    n = confs.shape[1]
    pt = torch.tensor(confs, device="cuda:0")
    ft = torch.full((B, n, 3), 2.0, dtype=torch.float64, device="cuda:0")
    et = torch.full((B,), 3.0, dtype=torch.float64, device="cuda:0")
    qt = torch.full((B, n), 4.0, dtype=torch.float64, device="cuda:0")
    ptr = lambda t: C.c_void_p(t.data_ptr())
    stats = k.batch_stats()
    assert lib.cf_compute_batch(k._h, 0, ptr(pt), 3, ptr(ft), ptr(et), ptr(qt)) == _cabi.CF_OK
    k.synchronize()
    assert k.batch_stats() == stats
    assert (ft == 2.0).all() and (et == 3.0).all() and (qt == 4.0).all()
    e0, f0, q0 = k.execute_batch_host(np.zeros((0, n, 3)))
    assert e0.shape == (0,) and f0.shape == (0, n, 3) and q0.shape == (0, n)
    # negative nconf, null positions
    assert lib.cf_compute_batch(k._h, -1, ptr(pt), 3, ptr(ft), ptr(et), ptr(qt)) == _cabi.CF_ERR_INVALID
    assert lib.cf_compute_batch(k._h, B, None, 3, ptr(ft), ptr(et), ptr(qt)) == _cabi.CF_ERR_INVALID
    assert lib.cf_compute_batch_host(k._h, B, None, 3, None, None, None) == _cabi.CF_ERR_INVALID
    assert lib.cf_set_batch_limit(k._h, -1) == _cabi.CF_ERR_INVALID
    assert (ft == 2.0).all() and (et == 3.0).all() and (qt == 4.0).all()
    # between cf_compute_begin and _end
    k.begin(pt[0])
    with pytest.raises(ChargeFluxError) as ei:
        k.execute_batch_device(pt, True, True, ft, et, qt)
    assert ei.value.code == _cabi.CF_ERR_STATE
    k.end()
    k.synchronize()
    # several ranks
    system, force, confs2, _ = _case(64, 64)
    k2 = HipCalcCoulForceKernel(rank=0, world_size=2).initialize(system, force)
    with pytest.raises(ChargeFluxError) as ei:
        k2.execute_batch_host(confs2)
    assert ei.value.code == _cabi.CF_ERR_STATE
