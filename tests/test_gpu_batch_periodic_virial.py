"""GPU tests of the virial tensors of the periodic batch (cf_compute_batch_periodic_virial,
include/chargeflux.h; DESIGN.md "Batched, periodic, virial").  Systems, boxes and conformations: the
recipes of test_gpu_batch_periodic_vjp.py (B = 3 boxes scaled per axis, in conformation 1 every fifth
atom moved by a whole box vector).  The yardstick is the complex step through
tests/pbc_virial_reference.py (guarded on the CPU by test_batch_periodic_virial_cpu.py).
Condition on the inputs (asserted, not a tolerance): no non-excluded minimum-image pair within 1e-9 nm
of the cutoff and no minimum-image component within 1e-9 nm of a face.
Bar of test 1: max|virial - ref| <= 1e-9 S + 1e-9 over the whole (B,3,3) array, S the sum over the
reference's parts (pairs, exclusions, self, reciprocal) of that part's largest absolute entry: the
parts cancel, so the rounding error scales with them and not with the total; 1e-9 is the bar of the
project's closed-form derivative calls against a complex step.  Observed on MI355X: see DESIGN.md.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import Oracle  # noqa: E402
from openmmcoul import ChargeFluxError, HipCalcCoulForceKernel, _cabi  # noqa: E402
from openmmcoul import testsystems as ts  # noqa: E402
from tests import pbc_virial_reference as vr  # noqa: E402
from tests.test_gpu_batch_periodic_vjp import (B, SYSTEMS, _assert_clear_of_cutoff, _conformations,  # noqa: E402
                                               _min_image, _system)

REL, ABS = 1e-9, 1e-9


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """(system, force, default box, conformations, boxes); the input condition."""
    system, force, pos, box = _system(name)
    confs, boxes = _conformations(name, pos, box, 400 + SYSTEMS.index(name))
    for x, bb in zip(confs, boxes):
        _assert_clear_of_cutoff(force, x, bb)
        d = _min_image(x[None, :, :] - x[:, None, :], bb)[~np.eye(len(x), dtype=bool)]
        assert np.abs(np.abs(d) - 0.5 * np.diag(bb)).min() > 1e-9
    return system, force, box, confs, boxes


@functools.lru_cache(maxsize=None)
def _expected(name):
    """(virials (B,3,3), S) of the reference."""
    system, force, box, confs, boxes = _inputs(name)
    ref = vr.Reference(force, *Oracle(force, box).ewald())
    parts = [ref.virial_parts(x, bb) for x, bb in zip(confs, boxes)]
    return np.stack([p["total"] for p in parts]), sum(max(np.abs(p[k]).max() for p in parts) for k in vr.PARTS)


def _kernel(name, **kw):
    system, force = _inputs(name)[:2]
    return HipCalcCoulForceKernel(**kw).initialize(system, force)


@pytest.mark.parametrize("name", ["w1", "ions", "w22", "aniso", "w100"])
def test_matches_the_complex_step_reference(name):
    system, force, box, confs, boxes = _inputs(name)
    k = _kernel(name)
    vir = k.execute_batch_virial_host(confs, boxes)[3]
    ref, scale = _expected(name)
    err = np.abs(vir - ref).max()
    print(f"{name}: max|virial - ref| = {err:.3e}, S = {scale:.3e}, max|ref| = {np.abs(ref).max():.3e}, "
          f"ratio = {err / scale:.3e}")
    assert vir.shape == (B, 3, 3) and np.isfinite(vir).all() and err <= REL * scale + ABS
    assert k.device_errors() == 0


@pytest.mark.parametrize("name", ["w22", "w100", "ions"])
def test_forward_outputs_are_bitwise_the_forward_call_s(name):
    system, force, box, confs, boxes = _inputs(name)
    k = _kernel(name)
    fwd = k.execute_batch_host(confs, boxes=boxes)
    out = k.execute_batch_virial_host(confs, boxes)
    assert all(np.array_equal(a, b) for a, b in zip(out[:3], fwd))
    assert np.array_equal(out[3], out[3].transpose(0, 2, 1)) and np.abs(out[3]).min() > 0
    assert k.device_errors() == 0


@pytest.mark.parametrize("name", ["w100", "ions"])
def test_bitwise_guarantees(name):
    stream = torch.cuda.Stream()
    system, force, box, confs, boxes = _inputs(name)
    k = _kernel(name, stream=stream.cuda_stream)
    run = lambda x, bb: k.execute_batch_virial_host(np.ascontiguousarray(x), np.ascontiguousarray(bb))
    stats = k.batch_stats()
    e, f, q, v = run(confs, boxes)
    assert k.batch_stats() == (stats[0] + 1, stats[1] + B, stats[2] + 1)   # one pass under the automatic limit
    for b in range(B):                                   # alone = its row of the batch
        assert np.array_equal(run(confs[b:b + 1], boxes[b:b + 1])[3][0], v[b])
    k.set_batch_limit(2)
    assert np.array_equal(run(confs, boxes)[3], v) and k.batch_stats()[2] == stats[2] + 1 + B + 2   # 2 + 1 conformations
    k.set_batch_limit(0)
    pt = torch.tensor(confs, device="cuda:0")
    ft = torch.zeros(confs.shape, dtype=torch.float64, device="cuda:0")
    et, qt = torch.empty(B, dtype=torch.float64, device="cuda:0"), torch.empty(q.shape, dtype=torch.float64, device="cuda:0")
    vt = torch.full((B, 3, 3), float("nan"), dtype=torch.float64, device="cuda:0")   # virials are overwritten
    torch.cuda.synchronize()   # the inputs exist before the side stream reads them
    bx = boxes.copy()
    k.execute_batch_virial_device(pt, True, True, ft, et, qt, vt, boxes=bx)
    bx[:] = np.nan             # the boxes are the caller's again as soon as the call returns
    stream.synchronize()
    assert all(np.array_equal(t.cpu().numpy(), a) for t, a in ((et, e), (ft, f), (qt, q), (vt, v)))
    assert k.device_errors() == 0


def test_argument_errors():
    system, force, cpos, _ = ts.cluster_c1()             # a non-periodic handle
    kn = HipCalcCoulForceKernel().initialize(system, force)
    with pytest.raises(ChargeFluxError) as ei:
        kn.execute_batch_virial_host(np.ascontiguousarray(cpos[None]), np.eye(3) * 3.0)
    assert ei.value.code == _cabi.CF_ERR_INVALID and "periodic" in str(ei.value)
    system, force, box, confs, boxes = _inputs("w22")
    k = _kernel("w22")
    k.execute_batch_virial_host(confs, boxes)
    stats = k.batch_stats()
    pt = torch.tensor(confs, device="cuda:0")
    outs = [torch.full(s, 2.0, dtype=torch.float64, device="cuda:0") for s in (confs.shape, (B,), confs.shape[:2], (B, 3, 3))]
    bad = boxes.copy()                                   # conformation 1 triclinic: `tric`'s shears, reduced form
    bad[1][1, 0], bad[1][2, 0], bad[1][2, 1] = 0.3 * bad[1][0, 0], -0.25 * bad[1][0, 0], 0.2 * bad[1][1, 1]
    for call in (lambda: k.execute_batch_virial_device(pt, True, True, *outs, boxes=bad),
                 lambda: k.execute_batch_virial_host(confs, bad)):
        with pytest.raises(ChargeFluxError) as ei:
            call()
        assert ei.value.code == _cabi.CF_ERR_INVALID and "conformation 1" in str(ei.value) and "triclinic" in str(ei.value)
        k.synchronize()
        assert all(bool((t == 2.0).all()) for t in outs) and k.batch_stats() == stats
    assert k.device_errors() == 0
