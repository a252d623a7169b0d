"""Cost of the electrostatic potential of a batch at probe points, on C1 (testsystems.cluster_c1, 256
atoms, non-periodic, P = 608 parameters): B distinct conformations (seeded jitter of the C1
positions, generated here), M distinct points each (testsystems.probe_points: seeded uniform draws in
the conformation's bounding box grown by 0.3 nm, a draw within 0.05 nm of an atom redrawn), through

  (a) forward:  one cf_compute_batch_esp (potentials and charges),
  (b) gradient: one cf_compute_batch_esp_vjp with a seeded normal cotangent, and
  (c) charges:  one cf_compute_batch with flags 0 and the charges output -- the flux and charge
                stages alone, which (a) runs before its own kernel,

on the same handle and the same device buffers.  After a warm-up of the three arms they are timed in
turn, `--repeats` times each (at least 5), a host clock around the call and the stream synchronise
that ends it.  Prints one JSON line: the per-conformation time of each arm (median, min and max over
the repeats) and the pair evaluations per second they amount to (B M N over the median; for the
forward arm after subtracting the charges arm's median).

  python tools/batch_esp_probe.py [--nconf 1024] [--npts 1024] [--repeats 7] [--out profiles/batch_esp_probe.json]
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
ap.add_argument("--npts", type=int, default=1024)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--seed", type=int, default=ts.SEED)
ap.add_argument("--out", default=None, help="also write the JSON line to this file")
args = ap.parse_args()
if args.repeats < 5:
    ap.error("--repeats must be at least 5")
if not torch.cuda.is_available():
    sys.exit("batch_esp_probe needs a HIP device")

system, force, pos, _ = ts.cluster_c1()
n, nb, m = len(pos), args.nconf, args.npts
rng = np.random.default_rng(args.seed)
confs = pos[None] + rng.normal(0.0, 0.003, size=(nb, n, 3))
points, _ = ts.probe_points(confs, m, args.seed + 1)

stream = torch.cuda.current_stream().cuda_stream
k = HipCalcCoulForceKernel(stream=stream).initialize(system, force)
lib = _cabi.load_library()
nparam = sum(k.param_counts())
dev = lambda a: torch.tensor(a, dtype=torch.float64, device="cuda")
zeros = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")
pt, rt, vbar = dev(confs), dev(points), dev(rng.normal(size=(nb, m)))
esp, chg, grad = zeros(nb, m), zeros(nb, n), zeros(nb, nparam)
ptr = lambda t: C.c_void_p(t.data_ptr())
a_pos, a_pts, a_vb, a_esp, a_chg, a_grad = (ptr(t) for t in (pt, rt, vbar, esp, chg, grad))
h, sync = k._h, lib.cf_synchronize


def timed(call):
    t0 = time.perf_counter()
    _cabi.check(call(), lib)
    _cabi.check(sync(h), lib)
    return time.perf_counter() - t0


arms = {
    "forward": lambda: lib.cf_compute_batch_esp(h, nb, a_pos, m, a_pts, a_esp, a_chg),
    "gradient": lambda: lib.cf_compute_batch_esp_vjp(h, nb, a_pos, m, a_pts, a_vb, a_grad),
    "charges": lambda: lib.cf_compute_batch(h, nb, a_pos, 0, None, None, a_chg),
}


def spread(ts_):
    us = [1e6 * t / nb for t in ts_]
    return {"median": statistics.median(us), "min": min(us), "max": max(us)}


for call in arms.values():       # warm-up of every arm (the workspace grows here)
    timed(call)
torch.cuda.synchronize()
times = {name: [] for name in arms}
for _ in range(args.repeats):    # in turn
    for name, call in arms.items():
        times[name].append(timed(call))
assert torch.isfinite(esp).all() and torch.isfinite(grad).all()
s = {name: spread(t) for name, t in times.items()}
pairs = float(m) * n   # per conformation
result = {"probe": "batch_esp_probe", "system": "C1", "atoms": n, "parameters": nparam, "nconf": nb, "npts": m,
          "repeats": args.repeats, "device": torch.cuda.get_device_name(0),
          "unit": "microseconds per conformation, wall time including the closing synchronise",
          "forward_us_per_conf": s["forward"], "gradient_us_per_conf": s["gradient"],
          "charges_us_per_conf": s["charges"],
          "forward_pairs_per_s": 1e6 * pairs / (s["forward"]["median"] - s["charges"]["median"]),
          "gradient_pairs_per_s": 1e6 * pairs / s["gradient"]["median"], "batch_stats": k.batch_stats()}
line = json.dumps(result)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
k.destroy()
