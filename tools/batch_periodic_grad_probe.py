"""Cost of the parameter gradients of a periodic batch against the batch itself, on the 64-water
system of tools/batch_periodic_probe.py (testsystems.water_box(64, cutoff=0.55), 192 atoms, kmax
7 x 7 x 7, P = 518 parameters): B distinct frames (seeded jitter of the positions, the box scaled per
axis by factors in [0.95, 1.05] with the positions scaled along, generated here) through

  (a) forward:  one cf_compute_batch_periodic (forces + energies), and
  (b) gradient: one cf_compute_batch_periodic_vjp with all three cotangents (seeded normal values),

on the same handle and the same device buffers.  After a warm-up of both arms the two are timed
alternately, `--repeats` times each (at least 5), a host clock around the call and the stream
synchronise that ends it.  Prints one JSON line: per B the per-conformation time of both arms (median,
min and max over the repeats) and their ratio.

Without cf_compute_batch_periodic_vjp the only route to the same gradient is central differences:
two forward batch calls per parameter, 2 P = 1036 of them.  That cost is stated as the measured
forward time x 2 P -- arithmetic on the forward arm's median, not a separate run.

  python tools/batch_periodic_grad_probe.py [--nconf 1024] [--repeats 7] [--out profiles/batch_periodic_grad_probe.json]
  python tools/batch_periodic_grad_probe.py --only 1024 --repeats 5      # one size (for a kernel trace)
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
ap.add_argument("--only", type=int, default=0, help="time this batch size alone")
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--seed", type=int, default=ts.SEED)
ap.add_argument("--out", default=None, help="also write the JSON line to this file")
args = ap.parse_args()
if args.repeats < 5:
    ap.error("--repeats must be at least 5")
if not torch.cuda.is_available():
    sys.exit("batch_periodic_grad_probe needs a HIP device")

system, force, pos, box = ts.water_box(64, cutoff=0.55)
n = len(pos)
sizes = [args.only] if args.only else sorted({1, 64, args.nconf})
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
frc = torch.zeros_like(pt)
ene = torch.zeros(bmax, dtype=torch.float64, device="cuda")
e_bar, q_bar, f_bar = dev(rng.normal(size=bmax)), dev(rng.normal(size=(bmax, n))), dev(rng.normal(size=(bmax, n, 3)))
grad = torch.zeros((bmax, nparam), dtype=torch.float64, device="cuda")
flags = _cabi.CF_INCLUDE_FORCES | _cabi.CF_INCLUDE_ENERGY
ptr = lambda t: C.c_void_p(t.data_ptr())
a_pos, a_frc, a_ene, a_eb, a_qb, a_fb, a_grad = (ptr(t) for t in (pt, frc, ene, e_bar, q_bar, f_bar, grad))
boxes_p = boxes.ctypes.data_as(C.POINTER(C.c_double))
h, sync = k._h, lib.cf_synchronize
compute_batch, compute_vjp = lib.cf_compute_batch_periodic, lib.cf_compute_batch_periodic_vjp


def forward(nb):
    t0 = time.perf_counter()
    _cabi.check(compute_batch(h, nb, a_pos, boxes_p, flags, a_frc, a_ene, None), lib)
    _cabi.check(sync(h), lib)
    return time.perf_counter() - t0


def gradient(nb):
    t0 = time.perf_counter()
    _cabi.check(compute_vjp(h, nb, a_pos, boxes_p, a_eb, a_qb, a_fb, a_grad), lib)
    _cabi.check(sync(h), lib)
    return time.perf_counter() - t0


def spread(ts_, nb):
    us = [1e6 * t / nb for t in ts_]
    return {"median": statistics.median(us), "min": min(us), "max": max(us)}


result = {"probe": "batch_periodic_grad_probe", "system": "water_box(64, cutoff=0.55)", "atoms": n,
          "parameters": nparam, "repeats": args.repeats, "device": torch.cuda.get_device_name(0),
          "cotangents": "energy, charges and forces",
          "unit": "microseconds per conformation, wall time including the closing synchronise", "sizes": {}}
for nb in sizes:
    forward(nb), gradient(nb)        # warm-up of both arms at this size (the workspaces grow here)
    torch.cuda.synchronize()
    tf, tg = [], []
    for _ in range(args.repeats):    # alternating
        tf.append(forward(nb))
        tg.append(gradient(nb))
    sf, sg = spread(tf, nb), spread(tg, nb)
    assert torch.isfinite(grad[:nb]).all()
    result["sizes"][str(nb)] = {
        "forward_us_per_conf": sf, "gradient_us_per_conf": sg,
        "ratio_gradient_over_forward": sg["median"] / sf["median"],
        "finite_difference_route_us_per_conf_forward_median_x_2P": sf["median"] * 2 * nparam,
        "finite_difference_route_over_gradient": sf["median"] * 2 * nparam / sg["median"],
    }
result["batch_stats"] = k.batch_stats()
line = json.dumps(result)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
k.destroy()
