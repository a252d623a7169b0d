"""Cost of the Hessian-vector products of a batch, on C1 (testsystems.cluster_c1, 256 atoms,
non-periodic): B distinct conformations (seeded jitter of the C1 positions, generated here) through

  (a) hvp_k1:   one cf_compute_batch_hvp with K = 1 direction per conformation,
  (b) hvp_k8:   one cf_compute_batch_hvp with K = 8 directions per conformation, and
  (c) forward:  one cf_compute_batch with both flags (energies, forces, charges) -- two of these per
                direction is what central differences of the forces would cost,

on the same handle and the same device buffers (seeded N(0, 1) directions).  After a warm-up of the
three arms they are timed in turn, `--repeats` times each (at least 5), a host clock around the call
and the stream synchronise that ends it.  Prints one JSON line: the time per (conformation,
direction) of each arm (median, min and max over the repeats; the forward arm per conformation) and
the ratio of each product arm's median to two forward batches.

  python tools/batch_hvp_probe.py [--nconf 1024] [--repeats 7] [--out profiles/batch_hvp_probe.json]
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
    sys.exit("batch_hvp_probe needs a HIP device")

system, force, pos, _ = ts.cluster_c1()
n, nb = len(pos), args.nconf
rng = np.random.default_rng(args.seed)
confs = pos[None] + rng.normal(0.0, 0.003, size=(nb, n, 3))

stream = torch.cuda.current_stream().cuda_stream
k = HipCalcCoulForceKernel(stream=stream).initialize(system, force)
lib = _cabi.load_library()
dev = lambda a: torch.tensor(a, dtype=torch.float64, device="cuda")
zeros = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")
ptr = lambda t: C.c_void_p(t.data_ptr())
pt = dev(confs)
vecs = {kk: dev(rng.normal(size=(nb, kk, n, 3))) for kk in KS}
outs = {kk: zeros(nb, kk, n, 3) for kk in KS}
frc, ene, chg = zeros(nb, n, 3), zeros(nb), zeros(nb, n)
h, sync = k._h, lib.cf_synchronize
flags = _cabi.CF_INCLUDE_FORCES | _cabi.CF_INCLUDE_ENERGY


def timed(call):
    t0 = time.perf_counter()
    _cabi.check(call(), lib)
    _cabi.check(sync(h), lib)
    return time.perf_counter() - t0


arms = {f"hvp_k{kk}": (lambda kk=kk: lib.cf_compute_batch_hvp(h, nb, ptr(pt), kk, ptr(vecs[kk]), ptr(outs[kk])))
        for kk in KS}
arms["forward"] = lambda: lib.cf_compute_batch(h, nb, ptr(pt), flags, ptr(frc), ptr(ene), ptr(chg))
rows = {f"hvp_k{kk}": nb * kk for kk in KS}
rows["forward"] = nb


def spread(name):
    us = [1e6 * t / rows[name] for t in times[name]]
    return {"median": statistics.median(us), "min": min(us), "max": max(us)}


for call in arms.values():       # warm-up of every arm (the workspaces grow here)
    timed(call)
torch.cuda.synchronize()
stats0 = k.batch_stats()
times = {name: [] for name in arms}
for _ in range(args.repeats):    # in turn
    for name, call in arms.items():
        times[name].append(timed(call))
stats1 = k.batch_stats()
assert all(torch.isfinite(o).all() for o in outs.values()) and torch.isfinite(frc).all()
result = {"probe": "batch_hvp_probe", "system": "C1", "atoms": n, "nconf": nb, "repeats": args.repeats,
          "device": torch.cuda.get_device_name(0),
          "unit": "microseconds per (conformation, direction) -- forward: per conformation -- wall time "
                  "including the closing synchronise"}
for name in arms:
    result[name + "_us"] = spread(name)
for kk in KS:
    result[f"hvp_k{kk}_over_two_forward"] = result[f"hvp_k{kk}_us"]["median"] / (2 * result["forward_us"]["median"])
result["passes_per_timed_round"] = (stats1[2] - stats0[2]) / args.repeats
line = json.dumps(result)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
k.destroy()
