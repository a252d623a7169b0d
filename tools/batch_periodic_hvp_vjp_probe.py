"""Cost of the parameter gradients of the periodic Hessian-vector products, on 64 waters
(testsystems.water_box(64), 192 atoms, cutoff 0.55 nm): B boxes (seeded jitter and per-axis box scaling
in [0.95, 1.05], generated here, the workload of tools/batch_periodic_hvp_probe.py) with K = 1 and K = 8
seeded N(0, 1) directions and cotangents per conformation through

  (a) vjp_k1, vjp_k8:  one cf_compute_batch_periodic_hvp_vjp, and
  (b) hvp_k1, hvp_k8:  one cf_compute_batch_periodic_hvp on the same positions, boxes and directions,

on the same handle and the same device buffers.  After a warm-up of the four arms they are timed in
turn, `--repeats` times each (at least 5), a host clock around the call and the stream synchronise that
ends it.  Prints one JSON line: the time per (conformation, direction) of each arm (median, min and max
over the repeats) and the ratio of the medians, gradient over product.  No pass / fail threshold.

  python tools/batch_periodic_hvp_vjp_probe.py [--nconf 1024] [--repeats 7] [--out profiles/batch_periodic_hvp_vjp_probe.json]
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

KS = (1, 8)

ap = argparse.ArgumentParser()
ap.add_argument("--nconf", type=int, default=1024)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--seed", type=int, default=ts.SEED)
ap.add_argument("--out", default=None, help="also write the JSON line to this file")
args = ap.parse_args()
if args.repeats < 5:
    ap.error("--repeats must be at least 5")
if not torch.cuda.is_available():
    sys.exit("batch_periodic_hvp_vjp_probe needs a HIP device")

system, force, pos, box = ts.water_box(64, cutoff=0.55)
n, nb = len(pos), args.nconf
rng = np.random.default_rng(args.seed)
scale = rng.uniform(0.95, 1.05, size=(nb, 3))
confs = (pos[None] + rng.normal(0.0, 0.003, size=(nb, n, 3))) * scale[:, None, :]
boxes = np.ascontiguousarray(box[None] * scale[:, None, :])

k = HipCalcCoulForceKernel(stream=torch.cuda.current_stream().cuda_stream).initialize(system, force)
lib = _cabi.load_library()
dev = lambda a: torch.tensor(a, dtype=torch.float64, device="cuda")
ptr = lambda t: C.c_void_p(t.data_ptr())
bp = boxes.ctypes.data_as(C.POINTER(C.c_double))
pt = dev(confs)
vecs = {kk: dev(rng.normal(size=(nb, kk, n, 3))) for kk in KS}
bars = {kk: dev(rng.normal(size=(nb, kk, n, 3))) for kk in KS}
outs = {kk: torch.zeros_like(vecs[kk]) for kk in KS}
grad = torch.zeros((nb, sum(k.param_counts())), dtype=torch.float64, device="cuda")
h = k._h


def timed(call):
    t0 = time.perf_counter()
    _cabi.check(call(), lib)
    _cabi.check(lib.cf_synchronize(h), lib)
    return time.perf_counter() - t0


arms, rows = {}, {}
for kk in KS:
    arms[f"vjp_k{kk}"] = lambda kk=kk: lib.cf_compute_batch_periodic_hvp_vjp(h, nb, ptr(pt), bp, kk, ptr(vecs[kk]),
                                                                             ptr(bars[kk]), ptr(grad))
    arms[f"hvp_k{kk}"] = lambda kk=kk: lib.cf_compute_batch_periodic_hvp(h, nb, ptr(pt), bp, kk, ptr(vecs[kk]),
                                                                         ptr(outs[kk]))
    rows[f"vjp_k{kk}"] = rows[f"hvp_k{kk}"] = nb * kk

for call in arms.values():       # warm-up of every arm (the workspaces grow here)
    timed(call)
torch.cuda.synchronize()
passes0 = k.batch_stats()[2]
times = {name: [] for name in arms}
for _ in range(args.repeats):    # in turn
    for name, call in arms.items():
        times[name].append(timed(call))
assert torch.isfinite(grad).all() and all(torch.isfinite(o).all() for o in outs.values())
result = {"probe": "batch_periodic_hvp_vjp_probe", "system": "64 waters, cutoff 0.55 nm", "atoms": n, "nconf": nb,
          "repeats": args.repeats, "passes_per_round": (k.batch_stats()[2] - passes0) // args.repeats,
          "device": torch.cuda.get_device_name(0),
          "unit": "microseconds per (conformation, direction), wall time including the closing synchronise"}
for name in arms:
    us = [1e6 * t / rows[name] for t in times[name]]
    result[name + "_us"] = {"median": statistics.median(us), "min": min(us), "max": max(us)}
for kk in KS:
    result[f"vjp_over_hvp_k{kk}"] = result[f"vjp_k{kk}_us"]["median"] / result[f"hvp_k{kk}_us"]["median"]
line = json.dumps(result)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
k.destroy()
