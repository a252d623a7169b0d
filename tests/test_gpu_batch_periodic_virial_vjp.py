"""GPU tests of cf_compute_batch_periodic_virial_vjp (include/chargeflux.h; DESIGN.md "Batched, periodic,
virial parameter gradients") on the frames of test_gpu_batch_periodic_virial.py (B = 3, its input
condition).  Yardstick: tests/pbc_virial_grad_reference.py, guarded by test_batch_periodic_virial_vjp_cpu.py.
Bar of test_matches_the_reference: max|grad - ref| <= 1e-9 G + 1e-9 per system, G the sum over the
reference's parts of the part's largest absolute gradient entry; 1e-9 is the project's bar for closed-form
derivative calls, and the reference's own noise (CPU guard: 3e-14 G) is far more than ten times below it.
All three frames of every system.  `w1`, `ions`, `w22`: every parameter.  `aniso`, `w100`: in frame b the
flat indices b, b + 8, ... and both ends of every group (flux rows: 70-73 of 518 and 108-109 of 810 a
frame; LJ rows over active_parameters: 18-20 of 128 and 28-29 of 200).  Observed on MI355X: see DESIGN.md.
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
from openmmcoul.fitting import BatchedChargeFlux  # noqa: E402
from tests import pbc_virial_grad_reference as gr  # noqa: E402
from tests import pbc_virial_reference as vr  # noqa: E402
from tests.lj_reference import active_parameters  # noqa: E402
from tests.test_gpu_batch_periodic_virial import _inputs, _kernel  # noqa: E402
from tests.test_gpu_batch_periodic_vjp import B, SYSTEMS, _counts  # noqa: E402

REL, ABS = 1e-9, 1e-9
SAMPLED = ("aniso", "w100")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _w_bar(name):
    return np.random.default_rng(90 + SYSTEMS.index(name)).normal(size=(B, 3, 3))


@functools.lru_cache(maxsize=None)
def _expected(name):
    """Per frame: (flux parameters, their per-part reference gradients, LJ parameters, theirs)."""
    system, force, box, confs, boxes = _inputs(name)
    ref = vr.Reference(force, *Oracle(force, box).ewald())
    counts, on, w, out = _counts(force), active_parameters(force), _w_bar(name), []
    for b in range(B):
        params, lj = list(range(sum(counts))), on
        if name in SAMPLED:
            params, lj = gr.strided(counts, 8, b), [on[i] for i in gr.strided((len(on) // 2, len(on) // 2), 8, b)]
        out.append((params, gr.theta_gradient(ref, confs[b], boxes[b], w[b], params),
                    lj, gr.lj_gradient(ref, confs[b], boxes[b], w[b], lj)))
    return out


@pytest.mark.parametrize("name", ["w1", "ions", "w22", "aniso", "w100"])
def test_matches_the_reference(name):
    system, force, box, confs, boxes = _inputs(name)
    k, want = _kernel(name), _expected(name)
    out = k.execute_batch_virial_vjp_host(confs, boxes, _w_bar(name), lj=True)
    assert out["flat"].shape == (B, sum(_counts(force))) and out["lj_flat"].shape == (B, 2 * len(confs[0]))
    assert np.isfinite(out["flat"]).all() and np.isfinite(out["lj_flat"]).all()
    for rows, got, at in (("flux", out["flat"], 0), ("lj", out["lj_flat"], 2)):
        err = max(np.abs(got[b][f[at]] - gr.total(f[at + 1])).max() for b, f in enumerate(want))
        G = gr.scale(*(f[at + 1] for f in want))
        print(f"{name} [{rows}]: {[len(f[at]) for f in want]} parameters of the {B} frames, "
              f"max|grad - ref| = {err:.3e}, G = {G:.3e}, ratio = {err / G if G else 0:.3e}")
        assert err <= REL * G + ABS, (name, rows, err, G)
    off = np.setdiff1d(np.arange(2 * len(confs[0])), active_parameters(force))
    assert not out["lj_flat"][:, off].any()              # eps = 0: exactly 0
    assert k.device_errors() == 0


@pytest.mark.parametrize("name", ["w22", "w100"])
def test_symmetry_and_linearity(name):
    system, force, box, confs, boxes = _inputs(name)
    k, w = _kernel(name), _w_bar(name)
    run = lambda wb: k.execute_batch_virial_vjp_host(confs, boxes, wb, lj=True)
    g, anti, tr, two = (run(np.ascontiguousarray(a)) for a in (w, w - w.transpose(0, 2, 1), w.transpose(0, 2, 1), 2 * w))
    for key in ("flat", "lj_flat"):
        assert not anti[key].any() and np.array_equal(tr[key], g[key])
        assert np.abs(g[key]).max() > 0 and np.abs(two[key] - 2 * g[key]).max() <= 1e-12 * np.abs(g[key]).max()
    stats = k.batch_stats()
    zero = run(None)                                     # no cotangent: exact zeros, counted, no pass
    gt = torch.full(g["flat"].shape, 7.0, dtype=torch.float64, device="cuda:0")
    lt = torch.full(g["lj_flat"].shape, 7.0, dtype=torch.float64, device="cuda:0")
    pt = torch.tensor(confs, device="cuda:0")
    k.execute_batch_virial_vjp_device(pt, boxes, gt, None, lt)
    k.execute_batch_virial_vjp_device(pt, boxes, None, torch.tensor(w, device="cuda:0"), None)   # nothing asked for
    k.synchronize()
    assert not zero["flat"].any() and not zero["lj_flat"].any() and not gt.any() and not lt.any()
    assert k.batch_stats() == (stats[0] + 3, stats[1] + 3 * B, stats[2])
    assert k.device_errors() == 0


@pytest.mark.parametrize("name", ["w100", "ions"])
def test_bitwise_guarantees(name):
    stream = torch.cuda.Stream()
    system, force, box, confs, boxes = _inputs(name)
    k, w = _kernel(name, stream=stream.cuda_stream), _w_bar(name)
    others = lambda: (*k.execute_batch_host(confs, boxes=boxes), *k.execute_batch_virial_host(confs, boxes),
                      k.execute_batch_vjp_host(confs, np.ones(B), boxes=boxes)["flat"])
    before = others()
    run = lambda rows, lj=True: k.execute_batch_virial_vjp_host(*(np.ascontiguousarray(a[rows]) for a in (confs, boxes, w)), lj=lj)
    same = lambda a, rows: np.array_equal(a["flat"], g["flat"][rows]) and np.array_equal(a["lj_flat"], g["lj_flat"][rows])
    stats = k.batch_stats()
    g = run(slice(None))
    assert k.batch_stats() == (stats[0] + 1, stats[1] + B, stats[2] + 1)   # one pass under the automatic limit
    for rows in [slice(b, b + 1) for b in range(B)] + [slice(None, None, -1)]:   # alone; the reversed batch
        assert same(run(rows), rows)
    passes = k.batch_stats()[2]
    k.set_batch_limit(1)
    assert same(run(slice(None)), slice(None)) and k.batch_stats()[2] == passes + B
    k.set_batch_limit(0)
    assert np.array_equal(run(slice(None), lj=False)["flat"], g["flat"])   # with or without the LJ rows
    pt, wt = torch.tensor(confs, device="cuda:0"), torch.tensor(w, device="cuda:0")
    gt, lt, l2 = (torch.full(g[key].shape, float("nan"), dtype=torch.float64, device="cuda:0")
                  for key in ("flat", "lj_flat", "lj_flat"))
    torch.cuda.synchronize()   # the inputs exist before the side stream reads them
    bx = boxes.copy()
    k.execute_batch_virial_vjp_device(pt, bx, gt, wt, lt)
    bx[:] = np.nan             # the boxes are the caller's again as soon as the call returns
    k.execute_batch_virial_vjp_device(pt, boxes, None, wt, l2)   # the LJ rows alone
    stream.synchronize()
    assert np.array_equal(gt.cpu().numpy(), g["flat"]) and all(np.array_equal(t.cpu().numpy(), g["lj_flat"]) for t in (lt, l2))
    assert all(np.array_equal(a, b) for a, b in zip(before, others()))
    assert k.device_errors() == 0


def test_argument_errors():
    lib = _cabi.load_library()
    system, force, cpos, _ = ts.cluster_c1()             # a non-periodic handle
    kn = HipCalcCoulForceKernel().initialize(system, force)
    with pytest.raises(ChargeFluxError, match="periodic") as ei:
        kn.execute_batch_virial_vjp_host(np.ascontiguousarray(cpos[None]), np.eye(3) * 3.0, np.ones((1, 3, 3)))
    assert ei.value.code == _cabi.CF_ERR_INVALID
    (system, force, box, confs, boxes), k, w = _inputs("w22"), _kernel("w22"), _w_bar("w22")
    g = k.execute_batch_virial_vjp_host(confs, boxes, w)["flat"]
    stats = k.batch_stats()
    pt, wt = torch.tensor(confs, device="cuda:0"), torch.tensor(w, device="cuda:0")
    gt = torch.full(g.shape, 2.0, dtype=torch.float64, device="cuda:0")

    def untouched():
        k.synchronize()
        return bool((gt == 2.0).all()) and k.batch_stats() == stats

    bad = boxes.copy()                                   # conformation 1 triclinic: `tric`'s shears, reduced form
    bad[1][1, 0], bad[1][2, 0], bad[1][2, 1] = 0.3 * bad[1][0, 0], -0.25 * bad[1][0, 0], 0.2 * bad[1][1, 1]
    for call in (lambda: k.execute_batch_virial_vjp_device(pt, bad, gt, wt), lambda: k.execute_batch_virial_vjp_host(confs, bad, w)):
        with pytest.raises(ChargeFluxError, match="conformation 1.*triclinic") as ei:
            call()
        assert ei.value.code == _cabi.CF_ERR_INVALID and untouched()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    gh = np.full(g.shape, 2.0)
    for fn, (p, wb, out) in ((lib.cf_compute_batch_periodic_virial_vjp, [C.c_void_p(t.data_ptr()) for t in (pt, wt, gt)]),
                             (lib.cf_compute_batch_periodic_virial_vjp_host, [dp(a) for a in (confs, w, gh)])):
        assert fn(k._h, B, None, dp(boxes), wb, out, None) == _cabi.CF_ERR_INVALID
        assert fn(k._h, B, p, None, wb, out, None) == _cabi.CF_ERR_INVALID
        assert fn(k._h, -1, p, dp(boxes), wb, out, None) == _cabi.CF_ERR_INVALID
        assert fn(k._h, 0, p, dp(boxes), wb, out, None) == _cabi.CF_OK
    assert untouched() and (gh == 2.0).all()
    k.begin(pt[0], boxes[0])                             # between cf_compute_begin and _end
    with pytest.raises(ChargeFluxError) as ei:
        k.execute_batch_virial_vjp_device(pt, boxes, gt, wt)
    k.end()
    assert ei.value.code == _cabi.CF_ERR_STATE and untouched()
    assert np.array_equal(k.execute_batch_virial_vjp_host(confs, boxes, w)["flat"], g)   # still works, the same bits
    assert k.device_errors() == 0
    k2 = HipCalcCoulForceKernel(rank=0, world_size=2).initialize(system, force)   # several ranks
    with pytest.raises(ChargeFluxError) as ei:
        k2.execute_batch_virial_vjp_host(confs, boxes, w)
    assert ei.value.code == _cabi.CF_ERR_STATE


@pytest.mark.parametrize("own_stream", [False, True])
def test_torch_layer(own_stream):
    """The loss reads the virials transposed, so their cotangent reaches backward non-contiguous."""
    system, force, box, confs, boxes = _inputs("w22")
    force, stream = copy.deepcopy(force), torch.cuda.Stream() if own_stream else None
    k = HipCalcCoulForceKernel(stream=stream.cuda_stream if own_stream else None).initialize(system, force)
    model = BatchedChargeFlux(k, force)
    pos = torch.tensor(confs, device="cuda:0")
    params, lj = model.parameters(device="cuda:0"), model.lj_parameters(device="cuda:0")
    virials = lambda: model.virials(*params, pos, boxes, sigmas=lj[0], epsilons=lj[1])
    out = virials()
    assert all(torch.equal(a, b) for a, b in zip(out[:3], model(*params, pos, boxes=boxes, sigmas=lj[0], epsilons=lj[1])))
    assert all(np.array_equal(t.detach().cpu().numpy(), a) for t, a in zip(out, k.execute_batch_virial_host(confs, boxes)))
    target = torch.tensor(np.random.default_rng(3).normal(size=(B, 3, 3)) * 100, device="cuda:0")
    w = np.ascontiguousarray((2 * (out[3] - target.mT)).detach().cpu().numpy())
    gv = k.execute_batch_virial_vjp_host(confs, boxes, w, lj=True)
    ge = (k.execute_batch_vjp_host(confs, np.ones(B), boxes=boxes)["flat"],
          k.execute_batch_lj_vjp_host(confs, np.ones(B), boxes=boxes)["flat"])
    for with_energy, ncalls in ((True, 3), (False, 1)):  # all three VJP calls; the virial VJP alone
        for p in params + lj:
            p.grad = None
        out = virials()
        calls = k.batch_stats()[0]
        (((out[3].mT - target) ** 2).sum() + (out[0].sum() if with_energy else 0.0)).backward()
        assert k.batch_stats()[0] == calls + ncalls
        for got, want in ((np.concatenate([p.grad.cpu().numpy().ravel() for p in params]), gv["flat"] + with_energy * ge[0]),
                          (np.concatenate([p.grad.cpu().numpy() for p in lj]), gv["lj_flat"] + with_energy * ge[1])):
            assert np.abs(got - want.sum(axis=0)).max() <= 1e-12 * np.abs(want.sum(axis=0)).max()
    calls = k.batch_stats()[0]
    model.virials(*params, pos, boxes)[0].sum().backward()   # the virials unused: no call for them
    assert k.batch_stats()[0] == calls + 2               # forward, periodic VJP
    with pytest.raises(ValueError):
        model.virials(*params, pos.clone().requires_grad_(True), boxes)
    assert k.device_errors() == 0
