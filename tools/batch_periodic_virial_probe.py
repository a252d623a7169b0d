"""What the virial tensors cost on top of the periodic forward batch: 64 waters
(testsystems.water_box(64, cutoff=0.55), 192 atoms, kmax 7 x 7 x 7), B distinct frames, each with its
own orthorhombic box (seeded jitter of the positions, the box scaled per axis by factors in
[0.95, 1.05] with the positions scaled along, generated here) through

  (a) forward: one cf_compute_batch_periodic, and
  (b) virial:  one cf_compute_batch_periodic_virial on the same inputs,

both with forces and energies, on the same handle and the same device buffers.  After a warm-up of
both arms the two are timed alternately, `--repeats` times each (at least 5), a host clock around the
call and the stream synchronise that ends it.  Prints one JSON line: per B the per-frame time of both
arms (median, min and max over the repeats), their ratio, whether the two ranges overlap, and whether
the two arms' energies and forces agree to the bit.

  python tools/batch_periodic_virial_probe.py [--nconf 1024] [--repeats 7] [--out profiles/batch_periodic_virial_probe.json]
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
    sys.exit("batch_periodic_virial_probe needs a HIP device")

system, force, pos, box = ts.water_box(64, cutoff=0.55)
n = len(pos)
sizes = sorted({1, 64, args.nconf})
bmax = sizes[-1]
rng = np.random.default_rng(args.seed)
scale = rng.uniform(0.95, 1.05, size=(bmax, 3))
confs = (pos[None] + rng.normal(0.0, 0.003, size=(bmax, n, 3))) * scale[:, None, :]
boxes = np.ascontiguousarray(box[None] * scale[:, None, :])

k = HipCalcCoulForceKernel(stream=torch.cuda.current_stream().cuda_stream).initialize(system, force)
lib = _cabi.load_library()
pt = torch.tensor(confs, dtype=torch.float64, device="cuda")
f_fwd, f_vir = torch.zeros_like(pt), torch.zeros_like(pt)
e_fwd = torch.zeros(bmax, dtype=torch.float64, device="cuda")
e_vir = torch.zeros_like(e_fwd)
vir = torch.zeros((bmax, 3, 3), dtype=torch.float64, device="cuda")
flags = _cabi.CF_INCLUDE_FORCES | _cabi.CF_INCLUDE_ENERGY
boxes_p = boxes.ctypes.data_as(C.POINTER(C.c_double))
ptr = lambda t: C.c_void_p(t.data_ptr())
h, sync = k._h, lib.cf_synchronize


def forward(nb):
    t0 = time.perf_counter()
    _cabi.check(lib.cf_compute_batch_periodic(h, nb, ptr(pt), boxes_p, flags, ptr(f_fwd), ptr(e_fwd), None), lib)
    _cabi.check(sync(h), lib)
    return time.perf_counter() - t0


def virial(nb):
    t0 = time.perf_counter()
    _cabi.check(lib.cf_compute_batch_periodic_virial(h, nb, ptr(pt), boxes_p, flags, ptr(f_vir), ptr(e_vir), None,
                                                     ptr(vir)), lib)
    _cabi.check(sync(h), lib)
    return time.perf_counter() - t0


def spread(ts_, nb):
    us = [1e6 * t / nb for t in ts_]
    return {"median": statistics.median(us), "min": min(us), "max": max(us)}


result = {"probe": "batch_periodic_virial_probe", "system": "water_box(64, cutoff=0.55)", "atoms": n,
          "repeats": args.repeats, "device": torch.cuda.get_device_name(0),
          "unit": "microseconds per frame, wall time including the closing synchronise", "sizes": {}}
for nb in sizes:
    forward(nb), virial(nb)          # warm-up of both arms at this size (the workspaces grow here)
    f_fwd.zero_(), f_vir.zero_()
    torch.cuda.synchronize()
    tf, tv = [], []
    for _ in range(args.repeats):    # alternating
        tf.append(forward(nb))
        tv.append(virial(nb))
    sf, sv = spread(tf, nb), spread(tv, nb)
    result["sizes"][str(nb)] = {
        "forward_us_per_frame": sf, "virial_us_per_frame": sv,
        "ratio_virial_over_forward": sv["median"] / sf["median"],
        "ranges_overlap": sv["min"] <= sf["max"] and sf["min"] <= sv["max"],
        "window_ms": {"forward": 1e3 * statistics.median(tf), "virial": 1e3 * statistics.median(tv)},
        # the same number of accumulating calls in both arms: the same bits
        "forces_and_energies_bitwise_equal": bool(torch.equal(f_fwd[:nb], f_vir[:nb]) and torch.equal(e_fwd[:nb], e_vir[:nb])),
        "virial_symmetric_and_finite": bool(torch.equal(vir[:nb], vir[:nb].transpose(1, 2)) and torch.isfinite(vir[:nb]).all()),
    }
result["batch_stats"] = k.batch_stats()
line = json.dumps(result)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
k.destroy()
