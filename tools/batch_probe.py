"""Batched against looped evaluation of many conformations of C1 (testsystems.cluster_c1, 256 atoms,
non-periodic): B distinct conformations (seeded jitter of the C1 positions, generated here) through

  (a) looped:  B device-resident cf_compute calls, one after the other, and
  (b) batched: one cf_compute_batch,

both with forces and energies, on the same handle and the same device buffers.  After a warm-up of
both arms the two are timed alternately, `--repeats` times each (at least 5), a host clock around
the calls and the stream synchronise that ends them.  Prints one JSON line: per B the
per-conformation time of both arms (median, min and max over the repeats), their ratio, and the
pair stage's work over the batched call's wall time -- two-sided pair evaluations per second and
the fp64 operations they stand for.  That is a rate over the wall time of the whole call (four
kernels and their launches), not the pair kernel's own rate and not a share of peak.

Operation count: one two-sided pair evaluation (cf_flux.h nopbc_pair, forces and energy) is 40 fp64
operations -- 3 for the distance vector, 5 for r^2, 1 sqrt, 1 division, 12 for the LJ and Coulomb
terms, 5 for the energy, 13 for the force and dE/dq -- counting sqrt and division as one each.  A
conformation is N (N - 1) - 2 X evaluations (X excluded pairs: each atom skips itself and its
excluded partners).

  python tools/batch_probe.py [--nconf 1024] [--repeats 7] [--out profiles/batch_probe.json]
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

OPS_PER_PAIR = 40

ap = argparse.ArgumentParser()
ap.add_argument("--nconf", type=int, default=1024)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--seed", type=int, default=ts.SEED)
ap.add_argument("--out", default=None, help="also write the JSON line to this file")
args = ap.parse_args()
if args.repeats < 5:
    ap.error("--repeats must be at least 5")
if not torch.cuda.is_available():
    sys.exit("batch_probe needs a HIP device")

system, force, pos, _ = ts.cluster_c1()
n = len(pos)
pairs = n * (n - 1) - 2 * force.getNumExceptions()
sizes = sorted({1, 64, args.nconf})
bmax = sizes[-1]
rng = np.random.default_rng(args.seed)
confs = pos[None] + rng.normal(0.0, 0.003, size=(bmax, n, 3))

stream = torch.cuda.current_stream().cuda_stream
k = HipCalcCoulForceKernel(stream=stream).initialize(system, force)
lib = _cabi.load_library()
pt = torch.tensor(confs, dtype=torch.float64, device="cuda")
f_loop, f_batch = torch.zeros_like(pt), torch.zeros_like(pt)
e_loop = torch.zeros(bmax, dtype=torch.float64, device="cuda")
e_batch = torch.zeros_like(e_loop)
flags = _cabi.CF_INCLUDE_FORCES | _cabi.CF_INCLUDE_ENERGY
box9 = (C.c_double * 9)()
# the looped arm's per-call arguments are made once: the timed loop is the C calls alone
loop_args = [(C.c_void_p(pt.data_ptr() + 24 * n * b), C.c_void_p(f_loop.data_ptr() + 24 * n * b),
              C.c_void_p(e_loop.data_ptr() + 8 * b)) for b in range(bmax)]
batch_args = (C.c_void_p(pt.data_ptr()), C.c_void_p(f_batch.data_ptr()), C.c_void_p(e_batch.data_ptr()))
h, compute, compute_batch, sync = k._h, lib.cf_compute, lib.cf_compute_batch, lib.cf_synchronize


def looped(nb):
    t0 = time.perf_counter()
    for p, f, e in loop_args[:nb]:
        rc = compute(h, p, box9, flags, f, e)
        if rc:
            _cabi.check(rc, lib)
    _cabi.check(sync(h), lib)
    return time.perf_counter() - t0


def batched(nb):
    t0 = time.perf_counter()
    _cabi.check(compute_batch(h, nb, batch_args[0], flags, batch_args[1], batch_args[2], None), lib)
    _cabi.check(sync(h), lib)
    return time.perf_counter() - t0


def spread(ts_, nb):
    us = [1e6 * t / nb for t in ts_]
    return {"median": statistics.median(us), "min": min(us), "max": max(us)}


result = {"probe": "batch_probe", "system": "C1", "atoms": n, "pair_evaluations_per_conformation": pairs,
          "fp64_ops_per_pair_evaluation": OPS_PER_PAIR, "repeats": args.repeats, "device": torch.cuda.get_device_name(0),
          "unit": "microseconds per conformation, wall time including the closing synchronise", "sizes": {}}
for nb in sizes:
    looped(nb), batched(nb)          # warm-up of both arms at this size (the batch workspace grows here)
    f_loop.zero_(), f_batch.zero_()
    torch.cuda.synchronize()
    tl, tb = [], []
    for _ in range(args.repeats):    # alternating
        tl.append(looped(nb))
        tb.append(batched(nb))
    # the same work: after the same number of accumulating calls the two arms hold the same forces
    df = (f_loop[:nb] - f_batch[:nb]).abs().max().item() / args.repeats
    de = (e_loop[:nb] - e_batch[:nb]).abs().max().item()
    sl, sb = spread(tl, nb), spread(tb, nb)
    wall = statistics.median(tb)
    result["sizes"][str(nb)] = {
        "looped_us_per_conf": sl, "batched_us_per_conf": sb,
        "ratio_looped_over_batched": sl["median"] / sb["median"],
        "batched_faster_beyond_spread": sb["max"] < sl["min"],
        "batched_pair_evaluations_per_s_over_wall_time": nb * pairs / wall,
        "batched_pair_fp64_ops_per_s_over_wall_time": nb * pairs * OPS_PER_PAIR / wall,
        "max_abs_force_difference_between_arms": df, "max_abs_energy_difference_between_arms": de,
    }
result["batch_stats"] = k.batch_stats()
line = json.dumps(result)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
k.destroy()
