"""Batched against looped evaluation of many periodic conformations, each with its own box: 64
waters (testsystems.water_box(64, cutoff=0.55), 192 atoms, kmax 7 x 7 x 7), B distinct conformations
(seeded jitter of the positions, the box scaled per axis by factors in [0.95, 1.05] with the
positions scaled along, generated here) through

  (a) looped:  B device-resident cf_compute calls, each with its conformation's box, on an
               exact-k-sum handle (kspace_algo 0), one after the other, and
  (b) batched: one cf_compute_batch_periodic,

both with forces and energies, on the same handle and the same device buffers.  After a warm-up of
both arms the two are timed alternately, `--repeats` times each (at least 5), a host clock around
the calls and the stream synchronise that ends them.  Prints one JSON line: per B the
per-conformation time of both arms (median, min and max over the repeats), their ratio, whether the
batched maximum lies below the looped minimum, and the largest difference between the two arms'
results.

  python tools/batch_periodic_probe.py [--nconf 1024] [--repeats 7] [--out profiles/batch_periodic_probe.json]
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
if args.repeats < 5:
    ap.error("--repeats must be at least 5")
if not torch.cuda.is_available():
    sys.exit("batch_periodic_probe needs a HIP device")

system, force, pos, box = ts.water_box(64, cutoff=0.55)
n = len(pos)
sizes = sorted({1, 64, args.nconf})
bmax = sizes[-1]
rng = np.random.default_rng(args.seed)
scale = rng.uniform(0.95, 1.05, size=(bmax, 3))
confs = (pos[None] + rng.normal(0.0, 0.003, size=(bmax, n, 3))) * scale[:, None, :]
boxes = np.ascontiguousarray(box[None] * scale[:, None, :])

stream = torch.cuda.current_stream().cuda_stream
k = HipCalcCoulForceKernel(stream=stream, kspace_algo=HipCalcCoulForceKernel.KSPACE_EXACT_MFMA).initialize(system, force)
lib = _cabi.load_library()
pt = torch.tensor(confs, dtype=torch.float64, device="cuda")
f_loop, f_batch = torch.zeros_like(pt), torch.zeros_like(pt)
e_loop = torch.zeros(bmax, dtype=torch.float64, device="cuda")
e_batch = torch.zeros_like(e_loop)
flags = _cabi.CF_INCLUDE_FORCES | _cabi.CF_INCLUDE_ENERGY
DP = C.POINTER(C.c_double)
boxes_p = boxes.ctypes.data_as(DP)
# the looped arm's per-call arguments are made once: the timed loop is the C calls alone
loop_args = [(C.c_void_p(pt.data_ptr() + 24 * n * b), C.cast(C.c_void_p(boxes.ctypes.data + 72 * b), DP),
              C.c_void_p(f_loop.data_ptr() + 24 * n * b), C.c_void_p(e_loop.data_ptr() + 8 * b)) for b in range(bmax)]
batch_args = (C.c_void_p(pt.data_ptr()), C.c_void_p(f_batch.data_ptr()), C.c_void_p(e_batch.data_ptr()))
h, compute, compute_batch, sync = k._h, lib.cf_compute, lib.cf_compute_batch_periodic, lib.cf_synchronize


def looped(nb):
    t0 = time.perf_counter()
    for p, b9, f, e in loop_args[:nb]:
        rc = compute(h, p, b9, flags, f, e)
        if rc:
            _cabi.check(rc, lib)
    _cabi.check(sync(h), lib)
    return time.perf_counter() - t0


def batched(nb):
    t0 = time.perf_counter()
    _cabi.check(compute_batch(h, nb, batch_args[0], boxes_p, flags, batch_args[1], batch_args[2], None), lib)
    _cabi.check(sync(h), lib)
    return time.perf_counter() - t0


def spread(ts_, nb):
    us = [1e6 * t / nb for t in ts_]
    return {"median": statistics.median(us), "min": min(us), "max": max(us)}


result = {"probe": "batch_periodic_probe", "system": "water_box(64, cutoff=0.55)", "atoms": n,
          "repeats": args.repeats,
          "device": torch.cuda.get_device_name(0),
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
    result["sizes"][str(nb)] = {
        "looped_us_per_conf": sl, "batched_us_per_conf": sb,
        "ratio_looped_over_batched": sl["median"] / sb["median"],
        "batched_faster_beyond_spread": sb["max"] < sl["min"],
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
