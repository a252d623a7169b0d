"""Cost of the parameter gradients of the virial tensors against the periodic parameter gradients, on
the 64-water system of tools/batch_periodic_grad_probe.py (testsystems.water_box(64, cutoff=0.55), 192
atoms, kmax 7 x 7 x 7, P = 518 parameters): B distinct frames, each in its own box (seeded jitter of
the positions, the box scaled per axis by factors in [0.95, 1.05] with the positions scaled along,
generated here) through

  (a) vjp:        one cf_compute_batch_periodic_vjp with all three cotangents,
  (b) virial:     one cf_compute_batch_periodic_virial_vjp, flux rows only, and
  (c) virial_lj:  the same call with the LJ rows too,

on the same handle, inputs and device buffers (seeded normal cotangents).  After a warm-up of the three
arms they are timed in turn, `--repeats` times each (at least 7), a host clock around the call and the
stream synchronise that ends it.  Prints one JSON line: per B the per-conformation time of each arm
(median, min and max over the repeats) and the ratios of (b) and (c) to (a).

  python tools/batch_periodic_virial_grad_probe.py [--nconf 1024] [--repeats 7] [--out profiles/batch_periodic_virial_grad_probe.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "openmm-chargeflux_amd")]
from openmmcoul import HipCalcCoulForceKernel, _cabi  # noqa: E402
from openmmcoul import testsystems as ts  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--nconf", type=int, default=1024)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--seed", type=int, default=ts.SEED)
ap.add_argument("--out", default=None, help="also write the JSON line to this file")
args = ap.parse_args()
if args.repeats < 7:
    ap.error("--repeats must be at least 7")
if not torch.cuda.is_available():
    sys.exit("batch_periodic_virial_grad_probe needs a HIP device")

system, force, pos, box = ts.water_box(64, cutoff=0.55)
n = len(pos)
sizes = sorted({1, 64, args.nconf})
bmax = sizes[-1]
rng = np.random.default_rng(args.seed)
scale = rng.uniform(0.95, 1.05, size=(bmax, 3))
confs = (pos[None] + rng.normal(0.0, 0.003, size=(bmax, n, 3))) * scale[:, None, :]
boxes = np.ascontiguousarray(box[None] * scale[:, None, :])

stream = torch.cuda.current_stream().cuda_stream
k = HipCalcCoulForceKernel(stream=stream).initialize(system, force)
lib = _cabi.load_library()
nparam = sum(k.param_counts())
dev = lambda a: torch.tensor(a, dtype=torch.float64, device="cuda")
pt = dev(confs)
e_bar, q_bar, f_bar = dev(rng.normal(size=bmax)), dev(rng.normal(size=(bmax, n))), dev(rng.normal(size=(bmax, n, 3)))
w_bar = dev(rng.normal(size=(bmax, 3, 3)))
grad = torch.zeros((bmax, nparam), dtype=torch.float64, device="cuda")
lj_grad = torch.zeros((bmax, 2 * n), dtype=torch.float64, device="cuda")
ptr = lambda t: C.c_void_p(t.data_ptr())
a_pos, a_eb, a_qb, a_fb, a_wb, a_grad, a_lj = (ptr(t) for t in (pt, e_bar, q_bar, f_bar, w_bar, grad, lj_grad))
boxes_p = boxes.ctypes.data_as(C.POINTER(C.c_double))
h, sync = k._h, lib.cf_synchronize
ARMS = {
    "vjp": lambda nb: lib.cf_compute_batch_periodic_vjp(h, nb, a_pos, boxes_p, a_eb, a_qb, a_fb, a_grad),
    "virial": lambda nb: lib.cf_compute_batch_periodic_virial_vjp(h, nb, a_pos, boxes_p, a_wb, a_grad, None),
    "virial_lj": lambda nb: lib.cf_compute_batch_periodic_virial_vjp(h, nb, a_pos, boxes_p, a_wb, a_grad, a_lj),
}


def timed(arm, nb):
    t0 = time.perf_counter()
    _cabi.check(ARMS[arm](nb), lib)
    _cabi.check(sync(h), lib)
    return time.perf_counter() - t0


def spread(ts_, nb):
    us = [1e6 * t / nb for t in ts_]
    return {"median": statistics.median(us), "min": min(us), "max": max(us)}


result = {"probe": "batch_periodic_virial_grad_probe", "system": "water_box(64, cutoff=0.55)", "atoms": n,
          "parameters": nparam, "repeats": args.repeats, "device": torch.cuda.get_device_name(0),
          "unit": "microseconds per conformation, wall time including the closing synchronise", "sizes": {}}
for nb in sizes:
    for arm in ARMS:                 # warm-up of every arm at this size (the workspaces grow here)
        timed(arm, nb)
    torch.cuda.synchronize()
    t = {arm: [] for arm in ARMS}
    for _ in range(args.repeats):    # alternating
        for arm in ARMS:
            t[arm].append(timed(arm, nb))
    s = {arm: spread(t[arm], nb) for arm in ARMS}
    assert torch.isfinite(grad[:nb]).all() and torch.isfinite(lj_grad[:nb]).all()
    result["sizes"][str(nb)] = {**{f"{arm}_us_per_conf": s[arm] for arm in ARMS},
                                "ratio_virial_over_vjp": s["virial"]["median"] / s["vjp"]["median"],
                                "ratio_virial_lj_over_vjp": s["virial_lj"]["median"] / s["vjp"]["median"]}
result["batch_stats"] = k.batch_stats()
line = json.dumps(result)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
k.destroy()
